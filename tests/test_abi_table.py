"""monte_carlo_localization_amd/abi.py against include/mcl_hip_engine.h, on the CPU: every signature of SIGNATURES against the
header's prototype, every structure and record dtype against the compiler's sizeof / offsetof, every mirrored constant against
the header's value, what the loader puts on the library against the table, and the names the engine module has always had."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcl_hip_engine.h")

C_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
             "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
C_RETURNS = dict(C_SCALARS, **{"void": None, "const char *": C.c_char_p})


def prototypes():
    """[(return type, name, [parameter text, ...])] of the header, in its order"""
    src = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = []
    for ret, name, params in re.findall(r"((?:const\s+)?\w+[\s\*]+)(mcl_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        ps = [" ".join(p.split()) for p in params.split(",")]
        out.append((" ".join(ret.split()), name, [] if ps in (["void"], [""]) else ps))
    return out


def is_pointer_type(t):
    return isinstance(t, type) and issubclass(t, C._Pointer)


def test_every_signature_is_the_headers(engine_mod):
    sig = engine_mod.SIGNATURES
    protos = prototypes()
    assert len(protos) == len(sig) == len({p[1] for p in protos})          # (a prototype the pattern misses fails here)
    assert [p[1] for p in protos] == list(sig) == engine_mod.EXPORTS       # the header's order
    wrong = []
    for ret, name, params in protos:
        restype, argtypes = sig[name]
        if ret not in C_RETURNS or restype is not C_RETURNS[ret]:
            wrong.append(f"{name}: returns `{ret}`, the table says {restype}")
        if len(params) != len(argtypes):
            wrong.append(f"{name}: {len(params)} parameters, the table has {len(argtypes)}")
            continue
        for i, (p, t) in enumerate(zip(params, argtypes)):
            words = re.sub(r"\bconst\b", " ", p).replace("*", " * ").replace("[", " [ ").split()
            where = f"{name}: parameter {i} `{p}`"
            if "*" in words or "[" in words:
                pointee = words[0]
                if t is C.c_void_p or t is C.c_char_p:
                    continue
                if not is_pointer_type(t):
                    wrong.append(f"{where} is a pointer, the table says {t.__name__}")
                elif issubclass(t._type_, C.Structure):
                    if getattr(t._type_, "_c_name_", None) != pointee:
                        wrong.append(f"{where}: the table points to {t._type_.__name__} ({getattr(t._type_, '_c_name_', None)})")
                elif pointee in C_SCALARS and words.count("*") == 1 and t._type_ is not C_SCALARS[pointee]:
                    wrong.append(f"{where}: the table points to {t._type_.__name__}")
            elif words[0] not in C_SCALARS:
                wrong.append(f"{where}: a scalar type this test does not know")
            elif t is not C_SCALARS[words[0]]:
                wrong.append(f"{where}: the table says {getattr(t, '__name__', t)}")
    assert not wrong, "\n".join(wrong)


# ---- one C99 probe for the layouts and the constants ------------------------------------------------------------------------------
# Python name -> header name, for the constants whose names differ by more than the MCL_ prefix
RENAMED = {"WEDGES": "MCL_WEDGES", "MAX_SEARCH_SCANS": "MCL_SEARCH_MAX_SCANS", "MAX_REFINE_SEQ_ROWS": "MCL_REFINE_SEQ_MAX_ROWS"}
PREFIXED = ("RESAMPLE_", "WEIGHT_", "RAYS_", "BUF_", "MOTION_")
# limits of the Python side that the header states in prose only (abi.py says so where it defines them)
NO_HEADER_MACRO = {"MAX_QUERY_POSES", "MAX_SEARCH_HITS", "MAX_REFINE_SEEDS", "MAX_REFINE_WINDOW"}
MAP_TABLE_IDS = {"grid": "MCL_MAP_TABLE_GRID", "skip": "MCL_MAP_TABLE_SKIP", "skip_nibbles": "MCL_MAP_TABLE_SKIP_NIBBLES",
                 "quadrant0": "MCL_MAP_TABLE_QUADRANT0", "free_cells": "MCL_MAP_TABLE_FREE_CELLS"}


def mirrored_constants(abi):
    """{header name: the Python value} of every integer constant of abi.py that mirrors one of the header"""
    out = {}
    for name, v in vars(abi).items():
        if not isinstance(v, int) or isinstance(v, bool) or name.startswith("_"):
            continue
        if name.startswith("MCL_"):
            out[name] = v
        elif name.startswith(PREFIXED):
            out["MCL_" + name] = v
        elif name in RENAMED:
            out[RENAMED[name]] = v
        else:
            assert name in NO_HEADER_MACRO, f"abi.{name}: neither mirrored from the header nor listed as having no macro there"
    for key, macro in MAP_TABLE_IDS.items():
        out[macro] = abi.MAP_TABLES[key][0]
    return out


def structures(abi):
    return [v for v in vars(abi).values() if isinstance(v, type) and issubclass(v, C.Structure)]


@pytest.fixture(scope="module")
def probe(engine_mod, tmp_path_factory):
    """{("S", type): sizeof, ("O", type, field): offsetof, ("Z", type, field): sizeof the field, ("K", name): value}, from gcc"""
    from monte_carlo_localization_amd import abi
    lines = []
    types = [(s._c_name_, [f[0] for f in s._fields_]) for s in structures(abi)]
    types += [(cname, list(dt.names)) for cname, dt in abi.RECORD_DTYPES.items()]
    for cname, fields in types:
        lines.append(f'printf("S {cname} %zu\\n", sizeof({cname}));')
        for f in fields:
            lines.append(f'printf("O {cname} {f} %zu\\n", offsetof({cname}, {f}));')
            lines.append(f'printf("Z {cname} {f} %zu\\n", sizeof((({cname} *)0)->{f}));')
    for macro in mirrored_constants(abi):
        lines.append(f'printf("K {macro} %lld\\n", (long long)({macro}));')
    d = tmp_path_factory.mktemp("abi_probe")
    src, exe = d / "probe.c", d / "probe"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcl_hip_engine.h"\nint main(void) {\n    '
                   + "\n    ".join(lines) + "\n    return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        *key, value = line.split()
        got[tuple(key)] = int(value)
    return got


def test_every_layout_is_the_compilers(engine_mod, probe):
    from monte_carlo_localization_amd import abi
    structs = structures(abi)
    assert len(structs) == 15 and len({s._c_name_ for s in structs}) == 15 and len(abi.RECORD_DTYPES) == 4
    wrong = []
    for s in structs:
        if C.sizeof(s) != probe["S", s._c_name_]:
            wrong.append(f"{s.__name__}: {C.sizeof(s)} bytes, {s._c_name_} has {probe['S', s._c_name_]}")
        for f, _ in s._fields_:
            have, want = (getattr(s, f).offset, getattr(s, f).size), (probe["O", s._c_name_, f], probe["Z", s._c_name_, f])
            if have != want:
                wrong.append(f"{s.__name__}.{f}: (offset, size) {have}, {s._c_name_} has {want}")
    for cname, dt in abi.RECORD_DTYPES.items():
        if dt.itemsize != probe["S", cname]:
            wrong.append(f"dtype of {cname}: {dt.itemsize} bytes, the type has {probe['S', cname]}")
        for f in dt.names:
            have, want = (dt.fields[f][1], dt.fields[f][0].itemsize), (probe["O", cname, f], probe["Z", cname, f])
            if have != want:
                wrong.append(f"dtype of {cname}, field {f}: (offset, size) {have}, the type has {want}")
    assert not wrong, "\n".join(wrong)


def test_every_mirrored_constant_is_the_headers(engine_mod, probe):
    from monte_carlo_localization_amd import abi
    consts = mirrored_constants(abi)
    assert len(consts) >= 30
    wrong = [f"{macro}: {v} in abi.py, {probe['K', macro]} in the header" for macro, v in consts.items() if v != probe["K", macro]]
    assert not wrong, "\n".join(wrong)
    # (the header names the first quadrant table and leaves the other three to a comment)
    q0 = abi.MAP_TABLES["quadrant0"][0]
    assert [abi.MAP_TABLES[f"quadrant{k}"][0] for k in range(4)] == [q0, q0 + 1, q0 + 2, q0 + 3]
    assert sorted(v[0] for v in abi.MAP_TABLES.values()) == list(range(8))
    assert abi.MOTION_MODELS == {"reference": abi.MOTION_REFERENCE, "diff": abi.MOTION_DIFF, "omni": abi.MOTION_OMNI}


@pytest.mark.parametrize("legacy", [False, True])
def test_the_loader_declares_every_function(engine_mod, legacy):
    lib = engine_mod.load_library(legacy=legacy)
    for name, (restype, argtypes) in engine_mod.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes), name


# the public names of monte_carlo_localization_amd.engine before it was divided into abi / host / engine / group, and the
# underscore helper that tools/ reach through it (tools/pose_query.py: engine._p)
ENGINE_NAMES = """
BUF_LOGW BUF_QWEIGHT BUF_SCALARS BUF_THETA BUF_X BUF_Y BeamSkipConfig BeamSkipState C CLUSTER_DTYPE Cluster ClusterConfig Config
EXPORTS Engine EngineError Group KldConfig LEGACY_LIB_PATH LIB_PATH LikelihoodFieldConfig MAP_TABLES MAX_QUERY_POSES
MAX_REFINE_SEEDS MAX_REFINE_SEQ_ROWS MAX_REFINE_WINDOW MAX_SEARCH_HITS MAX_SEARCH_SCANS MCL_ERR_INVALID_ARG MCL_ERR_NOT_READY
MCL_ERR_PEER MCL_ERR_TIMEOUT MCL_ERR_UNSUPPORTED MCL_OK MOTION_DIFF MOTION_MODELS MOTION_OMNI MOTION_REFERENCE MapPatchStats
MotionConfig POSE_SCORE_DTYPE PoseScore RAYS_AUTO RAYS_CELL RAYS_DESKEW RAYS_MARCH RAYS_QUAD RAYS_SKIP RAYS_SWEEP REFINE_DTYPE
RESAMPLE_MULTINOMIAL RESAMPLE_SYSTEMATIC RecoveryConfig RefineConfig SEARCH_HIT_DTYPE SORT_KEY_LOG2 SORT_MAX_FINE SearchConfig
SearchPruneConfig SearchStreamConfig ShardedUpdateError WEDGES WEDGE_R WEIGHT_LOG WEIGHT_PRODUCT annotations
default_beam_skip_config default_cluster_config default_config default_kld_config default_likelihood_field_config
default_motion_config default_recovery_config default_refine_config default_search_config host_beam_offset_pairs
host_beam_offset_table host_beam_skip_plan host_beam_skip_thresholds host_compact_guide host_compact_search host_gaussian_factor
host_kld_bins host_kld_target host_lf_pool host_likelihood_field host_likelihood_table host_map_patch_plan host_motion_sample
host_motion_scalars host_recovery_proposal host_recovery_step host_refine_reduce host_refine_sequence_offsets host_refine_window
host_scan_motion_offsets host_search_beam_grid host_search_blocks host_search_bound_table host_search_headings host_search_lattice
host_search_prune_next host_search_sequence_offsets host_search_slabs host_sensor_mount host_sensor_mount_cov host_sensor_table
host_sensor_unmount host_skip_field host_skip_field_dir host_skip_field_wedge host_skip_field_wedge_tight host_sort_key
host_sweep_global_layout host_wedge_tight_table load_library np os refine_window_size relative_poses search_prune_config
search_stream_config seed_counts sort_fine_code sort_tile_grid
_p
""".split()


def test_the_engine_module_keeps_its_names(engine_mod):
    assert len(ENGINE_NAMES) == 126
    missing = [n for n in ENGINE_NAMES if not hasattr(engine_mod, n)]
    assert not missing, missing
    from monte_carlo_localization_amd import abi, group, host
    for mod in (abi, host, group):               # engine re-exports every public name of the other three, as the same object
        for n, v in vars(mod).items():
            if not n.startswith("_"):
                assert getattr(engine_mod, n) is v, f"{mod.__name__}.{n}"
