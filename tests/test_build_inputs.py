"""What build() hashes to decide whether a built library is reused (__graft_entry__._hashed_inputs) covers what the units include:
a header missing from it would let build() reuse a stale library without saying so.  No GPU, nothing is compiled."""
import os
import re
import shutil

import pytest

import __graft_entry__ as g

INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def included_files():
    """Every file an #include "..." of csrc/ names that exists inside the repository (resolved from the including file)."""
    found = set()
    for name in sorted(os.listdir(g.CSRC)):
        path = os.path.join(g.CSRC, name)
        if not os.path.isfile(path) or not name.endswith((".hip", ".h")):
            continue
        for inc in INCLUDE.findall(open(path, encoding="utf-8").read()):
            target = os.path.realpath(os.path.join(g.CSRC, inc))
            if os.path.isfile(target) and target.startswith(os.path.realpath(g.ROOT) + os.sep):
                found.add(target)
    return sorted(found)


INCLUDED = included_files()


def test_every_included_file_is_hashed():
    assert len(INCLUDED) >= 30 and os.path.realpath(os.path.join(g.ROOT, "include", "mcl_hip_engine.h")) in INCLUDED
    hashed = {os.path.realpath(p) for p in g._hashed_inputs()}
    missing = [os.path.relpath(p, g.ROOT) for p in INCLUDED if p not in hashed]
    assert not missing, f"included by csrc/ but not hashed by build(): {missing}"
    units = {f for f in os.listdir(g.CSRC) if f.endswith(".hip")}
    assert set(g.SOURCES) == units and "mcl_engine.hip" in units


@pytest.fixture(scope="module")
def tree_copy(tmp_path_factory):
    root = tmp_path_factory.mktemp("inputs")
    shutil.copytree(g.CSRC, root / os.path.relpath(g.CSRC, g.ROOT), ignore=shutil.ignore_patterns("_build"))
    shutil.copytree(os.path.join(g.ROOT, "include"), root / "include")
    return str(root)


@pytest.mark.parametrize("rel", [os.path.relpath(p, os.path.realpath(g.ROOT)) for p in INCLUDED])
def test_one_changed_byte_of_a_header_changes_the_hash(tree_copy, rel):
    flags = [f for f in g.HIPCC_FLAGS if f != "-shared"]
    inputs = g._hashed_inputs(tree_copy)
    before = g._source_hash(inputs, flags, "toolchain")
    assert before == g._source_hash(g._hashed_inputs(), flags, "toolchain"), "the copy hashes like the tree"
    path = os.path.join(tree_copy, rel)
    data = open(path, "rb").read()
    try:
        open(path, "wb").write(bytes([data[0] ^ 1]) + data[1:])
        assert g._source_hash(inputs, flags, "toolchain") != before, rel
    finally:
        open(path, "wb").write(data)
