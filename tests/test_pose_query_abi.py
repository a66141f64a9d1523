"""The pose query's ABI (mcl_query_scans / mcl_score_poses) without a GPU: the header declares both calls and the
struct, engine.py binds them with matching argument types, the struct is 24 bytes on both sides, the libraries export the symbols."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcl_hip_engine.h")


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def prototype(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header_text())
    assert m, f"{name} is not declared in mcl_hip_engine.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


CTYPE_OF = [(r"^(const )?mcl_engine_t \*", C.c_void_p), (r"\*", C.c_void_p), (r"\[\d*\]$", C.c_void_p), (r"^int32_t ", C.c_int32), (r"^int64_t ", C.c_int64)]


def ctypes_of(args):
    out = []
    for a in args:
        for pat, t in CTYPE_OF:
            if re.search(pat, a):
                out.append(t)
                break
        else:
            raise AssertionError(f"no ctypes rule for '{a}'")
    return out


def test_header_declares_the_calls_and_the_struct():
    src = header_text()
    assert prototype("mcl_query_scans") == ["mcl_engine_t *h", "const double *poses_colmajor", "int32_t K", "float *ranges_m", "uint16_t *steps"]
    assert prototype("mcl_score_poses") == ["mcl_engine_t *h", "const double *poses_colmajor", "int32_t K", "const float *obs",
                                            "int32_t n_beams", "int32_t tol_steps", "mcl_pose_score_t *out"]
    m = re.search(r"typedef struct \{([^}]*)\} mcl_pose_score_t;", src)
    assert m
    fields = [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()]
    assert fields == ["double log_likelihood", "int32_t n_valid", "int32_t n_agree", "int32_t n_miss", "int32_t reserved"]
    for rule in ("Q1", "Q2", "Q3", "Q4", "Q5", "Q6"):
        assert re.search(r"\b" + rule + r"\b", open(HEADER).read()), rule


def test_engine_binds_them_with_matching_argtypes(engine_mod):
    for lib in (engine_mod.load_library(), engine_mod.load_library(legacy=True)):
        for name in ("mcl_query_scans", "mcl_score_poses", "mcl_get_query_counters"):
            assert name in engine_mod.EXPORTS
            assert list(getattr(lib, name).argtypes) == ctypes_of(prototype(name)), name
    assert hasattr(engine_mod.Engine, "expected_scans") and hasattr(engine_mod.Engine, "score_poses")


def test_struct_is_24_bytes_on_both_sides(engine_mod, tmp_path):
    S = engine_mod.PoseScore
    assert C.sizeof(S) == 24 and engine_mod.POSE_SCORE_DTYPE.itemsize == 24
    assert [(n, engine_mod.POSE_SCORE_DTYPE.fields[n][1]) for n in engine_mod.POSE_SCORE_DTYPE.names] == \
           [(n, getattr(S, n).offset) for n, _ in S._fields_]
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcl_hip_engine.h"\n'
                     'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mcl_pose_score_t), offsetof(mcl_pose_score_t, log_likelihood),'
                     'offsetof(mcl_pose_score_t, n_valid), offsetof(mcl_pose_score_t, n_agree), offsetof(mcl_pose_score_t, n_miss),'
                     'offsetof(mcl_pose_score_t, reserved));return 0;}\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(probe), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [24, S.log_likelihood.offset, S.n_valid.offset, S.n_agree.offset, S.n_miss.offset, S.reserved.offset]


def test_libraries_export_the_symbols_and_the_kernels(engine_mod):
    for path in (engine_mod.LIB_PATH, engine_mod.LEGACY_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in ("mcl_query_scans", "mcl_score_poses", "mcl_get_query_counters", "k_query_rays", "k_query_exact", "k_query_score"):
            assert name in out, (path, name)


def test_pose_argument_shapes(engine_mod):
    q = engine_mod.Engine._query_poses
    assert q([1.0, 2.0, 3.0]).shape == (3, 1) and q(np.zeros((5, 3))).shape == (3, 5)
    assert q(np.arange(6.0).reshape(2, 3)).tolist() == [[0.0, 3.0], [1.0, 4.0], [2.0, 5.0]]         # K x 3 column-major
    for bad in (np.zeros(4), np.zeros((3, 2)), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError):
            q(bad)
