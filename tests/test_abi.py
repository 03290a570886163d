"""The C-ABI surface without a GPU: the library loads, exports every symbol include/lcgs_hip.h declares, fails
loudly without a device (no CPU fallback), and its host-side helpers (scene ingest, synth scenes, image egress)
work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    return sorted(set(re.findall(r"LCGS_API\s+[\w\s\*]+?\b(lcgs_\w+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol(lcgs):
    lib = lcgs.load_library()
    declared = _declared_symbols()
    assert len(declared) >= 28
    for name in declared:
        assert hasattr(lib, name), f"liblcgs_hip.so does not export {name}"
    assert sorted(lcgs.api.EXPORTED_SYMBOLS) == declared, "api.EXPORTED_SYMBOLS out of sync with include/lcgs_hip.h"
    assert lib.lcgs_version().startswith(b"lcgs-hip")


# ---- the binding's declarations against the header ------------------------------------------------------------------
# C scalar -> the ctypes scalar the binding must declare for it (parameters, return values, struct members)
_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double,
            "char": C.c_char}
# pointees a struct member may also spell as a typed pointer (POINTER(c_float) for float*); c_void_p is always right
_POINTEES = dict(_SCALARS, uint32_t=C.c_uint32, int32_t=C.c_int32, uint8_t=C.c_uint8)
# structs with a body that deliberately have NO mirror: 128 opaque bytes the host carries between ranks in any buffer of
# that size; the binding takes lcgs_comm_id* as a plain address
_OPAQUE_STRUCTS = {"lcgs_comm_id"}


def _header():
    hdr = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return re.sub(r"//[^\n]*", " ", hdr)


def _header_constants(hdr):
    return {k: int(v) for k, v in re.findall(r"#define\s+(LCGS_\w+)\s+(\d+)\s*$", hdr, flags=re.M)}


def _expected_parameter(decl, structs):
    """one parameter declaration of a prototype -> the ctypes type the binding's conventions give it"""
    m = re.fullmatch(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)?\s*(\[\w*\])?", decl.strip())
    assert m, f"cannot parse parameter {decl!r}"
    base, stars, array = m.group(1), m.group(2).count("*"), m.group(4)
    if stars >= 2:  # handle out-parameters, arrays of pointers
        return C.POINTER(C.c_void_p)
    if stars == 0:
        return C.c_void_p if array else _SCALARS[base]  # `float x[3]` is an address
    if base == "char":
        return C.c_char_p
    if base in ("int", "int64_t"):  # host out-parameters
        return C.POINTER(_SCALARS[base])
    if base in structs:
        return C.POINTER(structs[base])
    return C.c_void_p  # opaque handles, device and host data, lcgs_comm_id*


def test_signature_table_matches_the_header(lcgs):
    """Every prototype of include/lcgs_hip.h against api.SIGNATURES: present, the return type, the number of parameters, and
    per parameter exactly the type the conventions in api._signatures' docstring give it (scalars by width, POINTER(mirror)
    for a struct with a mirror).  Then what load_library() put on the functions is the table."""
    api, hdr = lcgs.api, _header()
    protos = re.findall(r"LCGS_API\s+([\w\s\*]+?)\b(lcgs_\w+)\s*\(([^)]*)\)\s*;", hdr)
    assert sorted(n for _, n, _ in protos) == _declared_symbols() and len(protos) == len(set(n for _, n, _ in protos)) >= 89
    assert sorted(api.SIGNATURES) == _declared_symbols()
    restypes = {"lcgs_status": C.c_int, "void": None, "const char*": C.c_char_p, "int64_t": C.c_int64}
    lib = lcgs.load_library()
    for ret, name, params in protos:
        restype, argtypes = api.SIGNATURES[name]
        assert restype is restypes[" ".join(ret.split())], name
        decls = [] if params.strip() in ("", "void") else params.split(",")
        assert len(argtypes) == len(decls), f"{name}: {len(argtypes)} argtypes, {len(decls)} parameters"
        for k, decl in enumerate(decls):
            assert argtypes[k] is _expected_parameter(decl, api.STRUCTS), f"{name}, parameter {k} ({decl.strip()}): {argtypes[k]}"
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_struct_mirrors_match_the_header(lcgs):
    """Every struct the header defines with a body has a mirror in api.STRUCTS whose _fields_ are the header's members in
    order: name, scalar type, pointer-ness, array length (the header's integer #defines evaluated)."""
    api, hdr = lcgs.api, _header()
    consts = _header_constants(hdr)
    bodies = dict(re.findall(r"typedef\s+struct\s+(lcgs_\w+)\s*\{(.*?)\}\s*\1\s*;", hdr, flags=re.S))
    assert len(bodies) >= 16 and _OPAQUE_STRUCTS <= set(bodies)
    assert set(api.STRUCTS) == set(bodies) - _OPAQUE_STRUCTS
    for sname, body in bodies.items():
        if sname in _OPAQUE_STRUCTS:
            continue
        expected = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.match(r"(?:const\s+)?(\w+)\b(.*)", decl, flags=re.S)
            for declarator in m.group(2).split(","):
                d = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[([^\]]+)\])?\s*", declarator)
                assert d, f"{sname}: cannot parse {decl!r}"
                length = eval(d.group(3), {"__builtins__": {}}, consts) if d.group(3) else None
                expected.append((d.group(2), m.group(1), bool(d.group(1)), length))
        fields = api.STRUCTS[sname]._fields_
        assert [f[0] for f in fields] == [e[0] for e in expected], sname
        for (fname, ftype), (_, base, pointer, length) in zip(fields, expected):
            where = f"{sname}.{fname}"
            if length is not None:
                assert issubclass(ftype, C.Array) and ftype._length_ == length, where
                ftype = ftype._type_
            else:
                assert not issubclass(ftype, C.Array), where
            if not pointer:
                assert ftype is _SCALARS[base], where
            elif base == "char":
                assert ftype is C.c_char_p, where
            else:
                assert ftype in (C.c_void_p, C.POINTER(_POINTEES[base])), where
    assert (api.LCGS_MAX_STAGES, api.LCGS_MAX_RANKS, api.LCGS_ERR_STATE) == (consts["LCGS_MAX_STAGES"], consts["LCGS_MAX_RANKS"], 8)
    assert re.search(r"LCGS_ERR_STATE\s*=\s*8\b", hdr)


def test_declared_widths_reach_the_library(lcgs):
    """What the declarations buy: a bare Python int crosses as int64_t where the ABI says so, a bool is an int, and a wrapper
    of another width is refused instead of passed as it is."""
    assert lcgs.shard_rows(2 ** 40 + 3, 4, 1) == (2 ** 38, 2 ** 38)
    assert lcgs.api.owner_rows(2 ** 40 + 3, 4, 3) == (3 * 2 ** 38, 2 ** 38 + 3)
    lib = lcgs.load_library()
    assert lib.lcgs_sparse_message_words(2 ** 33, 3) == lcgs.api.sparse_message_words(2 ** 33, 3)
    assert lib.lcgs_owner_step_set_async(None, True) == 1  # LCGS_ERR_INVALID_ARG: NULL communicator
    first, count = C.c_int64(0), C.c_int64(0)
    with pytest.raises(C.ArgumentError):
        lib.lcgs_comm_shard_rows(C.c_int(10), 4, 3, C.byref(first), C.byref(count))
    with pytest.raises(C.ArgumentError):
        lib.lcgs_comm_shard_rows(10, 4, 3, C.byref(C.c_int(0)), C.byref(count))
    with pytest.raises(C.ArgumentError):
        lib.lcgs_set_fit_loss(None, 0.5, 0.2)  # a float where the ABI takes an int


def test_owner_step_that_never_settles_raises_lcgs_error(lcgs):
    """Comm.owner_step gives up after two repetitions with an LcgsError carrying LCGS_ERR_STATE (the three halves stubbed: no
    GPU, no communicator)."""

    class Stub:
        def __init__(self, short_steps):
            self.short_steps, self.calls = short_steps, []

        def owner_step_forward(self, *a):
            self.calls.append("forward")

        def owner_step_backward(self, *a):
            self.calls.append("backward")

        def owner_step_finish(self):
            self.short_steps -= 1
            return self.short_steps >= 0

    once = Stub(1)
    assert lcgs.Comm.owner_step(once, [], None, None, {}) == 1 and once.calls == ["forward", "backward"] * 2
    never = Stub(99)
    with pytest.raises(lcgs.LcgsError) as e:
        lcgs.Comm.owner_step(never, [], None, None, {})
    assert e.value.status == 8 and "did not settle" in str(e.value) and never.calls == ["forward", "backward"] * 3


def test_no_oracle_in_product():
    """The product never imports, links or calls the oracle (it is test infrastructure)."""
    pkg = os.path.join(ROOT, "luisacomputegaussiansplatting_amd")
    for dirpath, _, files in os.walk(pkg):
        if os.sep + "build" in dirpath or "__pycache__" in dirpath:
            continue
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in txt.lower(), f"{f} mentions the oracle"


def test_fails_loudly_without_gpu(lcgs):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(lcgs.LcgsError) as e:
        lcgs.Context(0)
    assert e.value.status == 3 and "no CPU path" in str(e.value)


def test_synth_scene_is_deterministic_and_counter_based(lcgs):
    a = lcgs.synth_scene(1, 2001, 5000)
    b = lcgs.synth_scene(1, 2001, 5000)
    c = lcgs.synth_scene(1, 2001, 1000, first=3000)
    d = lcgs.synth_scene(1, 2002, 5000)
    for k in a:
        assert np.array_equal(a[k], b[k])
        assert np.array_equal(a[k][3000:4000], c[k])  # any sub-range can be generated independently
        assert not np.array_equal(a[k], d[k])
    assert np.allclose(np.linalg.norm(a["rotq"], axis=1), 1, atol=1e-5)
    assert (a["opacity"] > 0).all() and (a["opacity"] < 1).all() and (a["scale"] > 0).all()
    obj = lcgs.synth_scene(0, 1001, 4000)
    assert np.linalg.norm(obj["pos"] - [0, 0, 0.5], axis=1).max() <= 1.2 + 1e-4


def test_ply_round_trip_and_errors(lcgs, tmp_path):
    rng = np.random.default_rng(0)
    P = 1000
    pos, f_dc, f_rest = rng.normal(size=(P, 3)), rng.normal(size=(P, 3)), rng.normal(size=(P, 45))
    op, ls, rot = rng.normal(size=P), rng.normal(-4, 1, (P, 3)), rng.normal(size=(P, 4))
    path = str(tmp_path / "scene.ply")
    lcgs.write_ply_raw(path, pos, f_dc, f_rest, op, ls, rot)
    s = lcgs.read_gs_ply(path)
    f32 = lambda x: np.asarray(x, np.float32)
    assert np.array_equal(s["pos"], f32(pos))
    assert np.array_equal(s["sh"].reshape(P, 16, 3)[:, 0, :], f32(f_dc))
    assert np.array_equal(s["sh"].reshape(P, 16, 3)[:, 1:, :], f32(f_rest).reshape(P, 3, 15).transpose(0, 2, 1))
    assert np.allclose(s["opacity"], 1 / (1 + np.exp(-f32(op))), rtol=3e-7)
    assert np.allclose(s["scale"], np.exp(f32(ls)), rtol=3e-7)
    assert np.allclose(np.linalg.norm(s["rotq"], axis=1), 1, atol=1e-6)
    # ascii PLY with a property missing -> format error (happly throws on a missing property, app/happly.h:974)
    bad = str(tmp_path / "bad.ply")
    with open(bad, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n0 0\n")
    with pytest.raises(lcgs.LcgsError) as e:
        lcgs.read_gs_ply(bad)
    assert e.value.status == 7
    with pytest.raises(lcgs.LcgsError) as e:
        lcgs.read_gs_ply(str(tmp_path / "missing.ply"))
    assert e.value.status == 6
    # empty vertex element
    empty = str(tmp_path / "empty.ply")
    lcgs.write_ply_raw(empty, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 45)), np.zeros(0), np.zeros((0, 3)),
                       np.zeros((0, 4)))
    assert lcgs.read_gs_ply(empty)["pos"].shape == (0, 3)


def test_png_writer(lcgs, tmp_path):
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    path = str(tmp_path / "out.png")
    lcgs.write_png(path, rgb)
    from PIL import Image

    back = np.array(Image.open(path))
    assert np.array_equal(back, rgb)


def test_comm_entry_points_without_a_gpu(lcgs):
    """The multi-GPU entry points that need no device: the rendezvous token (RCCL bound at run time -- the copy torch
    carries), row ownership, and argument checks that fail before anything touches a GPU."""
    import ctypes as C

    lib = lcgs.load_library()
    a, b = (C.c_char * 128)(), (C.c_char * 128)()
    st = lib.lcgs_comm_unique_id(a)
    if st == 0:  # RCCL present (it is in this image): two tokens differ, and are not all zeros
        assert lib.lcgs_comm_unique_id(b) == 0
        assert bytes(a.raw) != bytes(b.raw) and any(a.raw)
    else:  # no RCCL on this machine: a clean status and a message, nothing else breaks
        assert st == 3 and b"RCCL" in lib.lcgs_last_error()
    assert lib.lcgs_comm_unique_id(None) == 1  # LCGS_ERR_INVALID_ARG
    h = C.c_void_p(0)
    assert lib.lcgs_comm_create(None, a, C.c_int(0), C.c_int(1), C.byref(h)) == 1 and not h.value
    assert lib.lcgs_comm_destroy(None) == 0
    assert lcgs.shard_rows(10, 4, 3) == (6, 2)  # floor(10 / 4) rows each; rows 8, 9 are the tail every rank keeps
    # the ownership step's rows: equal contiguous shards, the tail with the LAST rank (= multi_gpu.owner_range)
    import luisacomputegaussiansplatting_amd.multi_gpu as mg

    for P, N in ((10, 4), (6_131_954, 8), (5, 8), (64, 1)):
        spans = [lcgs.api.owner_rows(P, N, r) for r in range(N)]
        assert spans == [mg.owner_range(P, N, r) for r in range(N)]
        assert spans[0][0] == 0 and sum(c for _, c in spans) == P and all(spans[r][0] + spans[r][1] == spans[r + 1][0] for r in range(N - 1))
    # the in-process loopback group needs no device either; the step's entry points refuse NULL arguments
    g = lcgs.api.LoopbackGroup(3)
    assert lib.lcgs_comm_create_loopback(None, g._h, C.c_int(0), C.byref(h)) == 1 and not h.value
    g.close()
    assert lib.lcgs_loopback_group_create(C.c_int(0), C.byref(h)) == 1  # world size out of range
    assert lib.lcgs_owner_step_forward(None, None, None, None, C.c_float(1.0), None) == 1
    assert lib.lcgs_owner_step_backward(None, None, None, None) == 1


def test_real_scene_env_hooks_switch_the_full_size_tests_to_the_file(lcgs, tmp_path, monkeypatch):
    """conftest.baseline_scene: LCGS_<NAME>_PLY pointing at a file makes a BASELINE scene `real` (read through
    lcgs_ply_read in the file's order), anything else the synthetic stand-in of SURVEY 8(d)."""
    from conftest import BASELINE_SCENES, baseline_scene

    assert set(BASELINE_SCENES) == {"lego", "chair", "bicycle", "garden"}
    rng = np.random.default_rng(4)
    P = 321
    path = str(tmp_path / "chair.ply")
    lcgs.write_ply_raw(path, rng.normal(0, 1, (P, 3)), rng.normal(0, 1, (P, 3)), rng.normal(0, 0.1, (P, 45)),
                       rng.normal(0, 1, P), rng.normal(-4, 1, (P, 3)), rng.normal(0, 1, (P, 4)))
    monkeypatch.setenv("LCGS_CHAIR_PLY", path)
    scene, data = baseline_scene(lcgs, "chair")
    assert data == "real" and scene["pos"].shape == (P, 3) and set(scene) == {"pos", "scale", "rotq", "sh", "opacity"}
    monkeypatch.setenv("LCGS_CHAIR_PLY", str(tmp_path / "missing.ply"))
    monkeypatch.setitem(BASELINE_SCENES, "chair", ("LCGS_CHAIR_PLY", 0, 1002, 500))  # (a small stand-in for this check)
    scene, data = baseline_scene(lcgs, "chair")
    assert data == "synthetic" and scene["pos"].shape == (500, 3)
