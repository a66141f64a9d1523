#!/usr/bin/env python3
"""Writes tests/golden/integration_patch_preimage.json: for every hunk of integration/particle_filter_hip.patch, the sha256 of
the lines of the reference checkout that the hunk replaces (its old range), and each target file's line count.  Digests only:
no line of the reference is stored.  tests/test_integration_patch.py checks the patch's own context and removed lines against
them, so the check that the diff applies needs no reference checkout.  Rerun after editing the patch:

    python tools/make_patch_fixture.py PATH_TO_REFERENCE_CHECKOUT
"""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "integration", "particle_filter_hip.patch")
OUT = os.path.join(ROOT, "tests", "golden", "integration_patch_preimage.json")


def lines_digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def patch_hunks(text):
    """{file: [(old_start, old_count), ...]} in patch order."""
    hunks, cur = {}, None
    for l in text.splitlines():
        m = re.match(r"^\+\+\+ b/(\S+)", l)
        if m:
            cur = hunks.setdefault(m.group(1), [])
            continue
        m = re.match(r"^@@ -(\d+)(?:,(\d+))? \+\d+(?:,\d+)? @@", l)
        if m:
            cur.append((int(m.group(1)), int(m.group(2) or 1)))
    return hunks


def main(reference):
    out = {}
    for f, hunks in patch_hunks(open(PATCH).read()).items():
        lines = open(os.path.join(reference, f)).read().splitlines()
        out[f] = {"lines": len(lines),
                  "hunks": [{"old_start": s, "old_count": c, "sha256": lines_digest(lines[s - 1:s - 1 + c])} for s, c in hunks]}
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
