"""The host patch as an artefact: integration/particle_filter_hip.patch is a unified diff against the
reference's src/particle_filter.cpp, include/particle_filter_cpp/particle_filter.hpp and CMakeLists.txt.  The diff must
apply cleanly to the reference (checked against digests of the reference's lines, tests/golden/integration_patch_preimage.json),
every C-ABI symbol it calls must be declared in include/mcl_hip_engine.h and exported by the built library, and the class
surface must be untouched apart from the four private additions."""
import hashlib
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "integration", "particle_filter_hip.patch")
PREIMAGE = os.path.join(ROOT, "tests", "golden", "integration_patch_preimage.json")


def patch_text():
    return open(PATCH).read()


def test_patch_touches_only_the_three_files():
    files = re.findall(r"^\+\+\+ b/(\S+)", patch_text(), flags=re.M)
    assert files == ["CMakeLists.txt", "include/particle_filter_cpp/particle_filter.hpp", "src/particle_filter.cpp"]


def test_every_engine_call_is_declared_in_the_header():
    added = "\n".join(l[1:] for l in patch_text().splitlines() if l.startswith("+") and not l.startswith("+++"))
    used = set(re.findall(r"\b(mcl_[a-z_]+)\s*\(", added))
    header = open(os.path.join(ROOT, "include", "mcl_hip_engine.h")).read()
    declared = set(re.findall(r"\b(mcl_[a-z_0-9]+)\s*\(", header))
    assert used and used <= declared, sorted(used - declared)
    assert {"mcl_create", "mcl_destroy", "mcl_set_map", "mcl_set_beam_angles", "mcl_set_particles", "mcl_update",
            "mcl_expected_pose", "mcl_get_stage_timings", "mcl_sample_particles", "mcl_particle_mean"} <= used


def test_class_surface_unchanged():
    """No public member, no existing private declaration and no signature is removed from the header: the only removed
    lines of the whole diff are the bodies of MCL() / expected_pose() and the visualisation draw they replace."""
    hunks = patch_text().split("+++ b/")
    hpp = next(h for h in hunks if h.startswith("include/particle_filter_cpp/particle_filter.hpp"))
    removed = [l for l in hpp.splitlines() if l.startswith("-") and not l.startswith("---")]
    assert removed == []
    added = [l[1:].strip() for l in hpp.splitlines() if l.startswith("+") and not l.startswith("+++") and l[1:].strip()]
    assert [a for a in added if not a.startswith("//")] == [
        '#include "mcl_hip_engine.h"', "~ParticleFilter() override;",
        "mcl_engine_t *engine_ = nullptr;  // libmcl_hip_engine.so: resample, motion, ray cast, table lookup, normalise, pose",
        "bool host_state_stale_ = false;   // particles_ / weights_ lag behind the engine until sync_host_state()",
        "void sync_host_state();", "void push_host_state();"]


def parse_hunks(text):
    """{file: [(old_start, old_count, new_start, new_count, old_lines, new_lines), ...]} of a unified diff."""
    files, cur, hunk = {}, None, None
    for l in text.splitlines():
        if l.startswith("--- a/"):
            continue
        if l.startswith("+++ b/"):
            cur, hunk = files.setdefault(l[6:].strip(), []), None
            continue
        m = re.match(r"^@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", l)
        if m:
            hunk = (int(m.group(1)), int(m.group(2) or 1), int(m.group(3)), int(m.group(4) or 1), [], [])
            cur.append(hunk)
            continue
        assert hunk is not None, l
        tag, body = (l[0], l[1:]) if l else (" ", "")
        assert tag in " -+", l
        if tag in " -":
            hunk[4].append(body)
        if tag in " +":
            hunk[5].append(body)
    return files


def test_patch_applies_to_the_reference():
    """`git apply --check` against the reference without its checkout: every hunk's body agrees with its header, the hunks
    lie in order inside the file and their new ranges follow from the old ones, and the lines each hunk replaces (its context
    and removed lines) hash to the digest of the reference's own lines at that place (tools/make_patch_fixture.py writes the
    digests from a reference checkout)."""
    want = json.load(open(PREIMAGE))
    got = parse_hunks(patch_text())
    assert sorted(got) == sorted(want)
    for f, hunks in got.items():
        ref = want[f]
        assert [(h[0], h[1]) for h in hunks] == [(r["old_start"], r["old_count"]) for r in ref["hunks"]], f
        end, delta = 0, 0
        for (o_start, o_count, n_start, n_count, old, new), r in zip(hunks, ref["hunks"]):
            assert (len(old), len(new)) == (o_count, n_count), (f, o_start)
            assert o_start > end and o_start - 1 + o_count <= ref["lines"], (f, o_start)
            assert n_start == o_start + delta, (f, o_start)
            assert hashlib.sha256("\n".join(old).encode()).hexdigest() == r["sha256"], (f, o_start)
            end, delta = o_start - 1 + o_count, delta + n_count - o_count
