"""The ABI of the pose refinement under the beam model (mcl_refine_poses_beam) without a GPU: the header declares
the call with the arguments of mcl_refine_poses and documents RB1-RB6, engine.py binds it with matching argument types, the
libraries export the symbol and the kernel, and a null engine is refused before any device is touched."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcl_hip_engine.h")
ARGS = ["mcl_engine_t *h", "const mcl_refine_config_t *c", "const double *seeds_colmajor", "int32_t M", "const float *obs",
        "int32_t n_beams", "mcl_refine_result_t *out"]


def prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in mcl_hip_engine.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_call_and_its_rules():
    assert prototype("mcl_refine_poses_beam") == ARGS + ["uint64_t stats[6]"]
    assert prototype("mcl_refine_poses") == ARGS + ["uint64_t stats[4]"]        # (the same config and result structs)
    text = open(HEADER).read()
    for rule in ("RB1", "RB2", "RB3", "RB4", "RB5", "RB6"):
        assert re.search(r"\b" + rule + r"\b", text), rule
    assert "refinement under the beam model, shards" not in text                  # B6's "Not here" line no longer lists it


def test_engine_binds_it_with_matching_argtypes(engine_mod):
    assert "mcl_refine_poses_beam" in engine_mod.EXPORTS
    for lib in (engine_mod.load_library(), engine_mod.load_library(legacy=True)):
        got = list(lib.mcl_refine_poses_beam.argtypes)
        assert got == [C.c_void_p, C.POINTER(engine_mod.RefineConfig), C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                       C.c_void_p]
        assert len(got) == len(prototype("mcl_refine_poses_beam"))
    assert hasattr(engine_mod.Engine, "refine_poses_beam")


def test_libraries_export_the_symbol_and_the_kernel(engine_mod):
    for path in (engine_mod.LIB_PATH, engine_mod.LEGACY_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        for name in ("mcl_refine_poses_beam", "k_refine_beam_score", "k_refine_beam_rows", "mcl_refine_poses", "k_refine_reduce"):
            assert name in out, (path, name)


def test_null_engine_is_refused_without_a_device(engine_mod):
    lib = engine_mod.load_library()
    cfg = engine_mod.default_refine_config()
    assert lib.mcl_refine_poses_beam(None, C.byref(cfg), None, 1, None, 1, None, None) == engine_mod.MCL_ERR_INVALID_ARG
    assert lib.mcl_refine_poses_beam(None, None, None, 0, None, 0, None, None) == engine_mod.MCL_ERR_INVALID_ARG
