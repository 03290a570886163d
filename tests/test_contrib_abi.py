"""Contribution-based pruning without a GPU: the three device entry points are exported, listed and declared, and refuse bad
arguments before anything touches a device; lcgs_ply_filter_rows (host only) copies the kept records of a binary PLY bit for bit
(with tests/test_abi.py this pins header <-> EXPORTED_SYMBOLS <-> liblcgs_hip.so)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

NAMES = ("lcgs_contrib_accumulate", "lcgs_contrib_keep_mask", "lcgs_prune", "lcgs_ply_filter_rows")
INVALID_ARG, IO, FORMAT = 1, 6, 7
TINY = os.path.join(GOLDEN, "tiny_scene.ply")


def _addr(k):
    return C.c_void_p(0x100000 * (k + 1))  # never dereferenced


def test_symbols_are_exported_listed_and_declared(lcgs):
    lib = lcgs.load_library()
    header = open(os.path.join(ROOT, "include", "lcgs_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in lcgs.api.EXPORTED_SYMBOLS, name
        assert re.search(r"LCGS_API\s+lcgs_status\s+" + name + r"\s*\(", header), name
    for method in ("contrib_accumulate", "contrib_keep_mask", "prune"):
        assert callable(getattr(lcgs.Renderer, method))
    assert callable(lcgs.ply_filter_rows)
    # what is not offered is said where the contract is
    for phrase in ("ownership step", "score while rendering", "gradient-weighted", "lcgs-app flag"):
        assert phrase in header, phrase


def test_contrib_accumulate_refuses_bad_arguments_before_any_device_work(lcgs):
    lib = lcgs.load_library()
    fn = lib.lcgs_contrib_accumulate
    null, ctx = C.c_void_p(0), C.c_void_p(0x1000)  # a non-NULL context that is never dereferenced
    full = lcgs.api._ContribStats(*[_addr(k) for k in range(4)])
    assert fn(null, 10, C.byref(full)) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, 10, None) == INVALID_ARG
    assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, 10, C.byref(lcgs.api._ContribStats())) == INVALID_ARG  # any member may be NULL, not all four
    assert b"all four" in lib.lcgs_last_error()


def _packs(lcgs, n=7):
    return [lcgs.api._Params(*[_addr(8 + 5 * j + k) for k in range(5)]) for j in range(n)]


def test_keep_mask_and_prune_refuse_bad_arguments_before_any_device_work(lcgs):
    lib, api = lcgs.load_library(), lcgs.api
    null, ctx, keep = C.c_void_p(0), C.c_void_p(0x1000), _addr(40)
    stats = api._ContribStats(*[_addr(k) for k in range(4)])
    cfg = api._PruneConfig(0.01, 0.0, 0, 0)
    fn = lib.lcgs_contrib_keep_mask
    for args in ((null, 10, C.byref(cfg), C.byref(stats), keep), (ctx, 10, None, C.byref(stats), keep),
                 (ctx, 10, C.byref(cfg), None, keep), (ctx, 10, C.byref(cfg), C.byref(stats), null)):
        assert fn(*args) == INVALID_ARG
        assert b"NULL" in lib.lcgs_last_error()
    assert fn(ctx, -1, C.byref(cfg), C.byref(stats), keep) == INVALID_ARG
    # a non-zero minimum whose statistics member is NULL, one member at a time
    for k, c in enumerate((api._PruneConfig(0.0, 0.5, 0, 0), api._PruneConfig(0.01, 0.0, 0, 0), api._PruneConfig(0.0, 0.0, 1, 0),
                           api._PruneConfig(0.0, 0.0, 0, 2))):
        ptrs = [_addr(j) for j in range(4)]
        ptrs[k] = null
        assert fn(ctx, 10, C.byref(c), C.byref(api._ContribStats(*ptrs)), keep) == INVALID_ARG, k
        assert b"minimum" in lib.lcgs_last_error()

    fn = lib.lcgs_prune
    packs, n = _packs(lcgs), C.c_int64(-5)
    refs = [C.byref(p) for p in packs]
    assert fn(null, 10, 3, C.byref(cfg), C.byref(stats), *refs, 10, null, C.byref(n)) == INVALID_ARG
    assert fn(ctx, 10, 3, None, C.byref(stats), *refs, 10, null, C.byref(n)) == INVALID_ARG
    assert fn(ctx, 10, 3, C.byref(cfg), None, *refs, 10, null, C.byref(n)) == INVALID_ARG
    assert fn(ctx, 10, 3, C.byref(cfg), C.byref(stats), *refs, 10, null, None) == INVALID_ARG
    for k in range(7):
        a = list(refs)
        a[k] = None
        assert fn(ctx, 10, 3, C.byref(cfg), C.byref(stats), *a, 10, null, C.byref(n)) == INVALID_ARG, k
    assert fn(ctx, -1, 3, C.byref(cfg), C.byref(stats), *refs, 10, null, C.byref(n)) == INVALID_ARG
    assert fn(ctx, 10, 4, C.byref(cfg), C.byref(stats), *refs, 10, null, C.byref(n)) == INVALID_ARG
    assert b"sh_degree" in lib.lcgs_last_error()
    assert fn(ctx, 10, 3, C.byref(cfg), C.byref(stats), *refs, -1, null, C.byref(n)) == INVALID_ARG
    assert b"capacity" in lib.lcgs_last_error()
    no_max = api._ContribStats(_addr(0), null, _addr(2), _addr(3))
    assert fn(ctx, 10, 3, C.byref(cfg), C.byref(no_max), *refs, 10, null, C.byref(n)) == INVALID_ARG
    assert b"minimum" in lib.lcgs_last_error()
    # a NULL member of a pack; destinations that alias their sources
    holed = _packs(lcgs)
    holed[3].scale = None
    assert fn(ctx, 10, 3, C.byref(cfg), C.byref(stats), *[C.byref(p) for p in holed], 10, null, C.byref(n)) == INVALID_ARG
    assert b"parameter pack" in lib.lcgs_last_error()
    alias = _packs(lcgs)
    alias[3].pos = alias[0].pos
    assert fn(ctx, 10, 3, C.byref(cfg), C.byref(stats), *[C.byref(p) for p in alias], 10, null, C.byref(n)) == INVALID_ARG
    assert b"out of place" in lib.lcgs_last_error()


# ---- lcgs_ply_filter_rows
def _payload(path):
    raw = open(path, "rb").read()
    at = raw.index(b"end_header\n") + len(b"end_header\n")
    return raw[:at], raw[at:]


def test_ply_filter_rows_copies_the_kept_records_bit_for_bit(lcgs, tmp_path):
    src = lcgs.read_gs_ply(TINY)
    P = src["pos"].shape[0]
    keep = np.random.default_rng(3).random(P) < 0.6
    keep[0], keep[-1] = False, True
    out = str(tmp_path / "pruned.ply")
    lcgs.ply_filter_rows(TINY, out, keep)
    got = lcgs.read_gs_ply(out)
    assert got["pos"].shape[0] == int(keep.sum()) and 0 < keep.sum() < P
    for k in ("pos", "sh", "opacity", "scale", "rotq"):
        assert np.array_equal(got[k].view(np.uint32), src[k][keep].view(np.uint32)), k
    # the records themselves, and a header that differs in the count's digits only
    head_in, data_in = _payload(TINY)
    head_out, data_out = _payload(out)
    stride = len(data_in) // P
    assert len(data_in) == P * stride
    assert data_out == b"".join(data_in[j * stride:(j + 1) * stride] for j in np.nonzero(keep)[0])
    assert head_out == head_in.replace(b"element vertex %d\n" % P, b"element vertex %d\n" % keep.sum())
    # a mask of any integer type counts non-zero entries; dropping everything leaves a valid empty file
    lcgs.ply_filter_rows(TINY, out, keep.astype(np.int32) * 7)
    assert _payload(out)[1] == data_out
    lcgs.ply_filter_rows(TINY, out, np.zeros(P, np.uint8))
    assert lcgs.read_gs_ply(out)["pos"].shape == (0, 3) and _payload(out)[1] == b""


def test_ply_filter_rows_keep_all_reproduces_the_file(lcgs, tmp_path):
    P = lcgs.read_gs_ply(TINY)["pos"].shape[0]
    out = str(tmp_path / "same.ply")
    lcgs.ply_filter_rows(TINY, out, np.ones(P, np.uint8))
    assert open(out, "rb").read() == open(TINY, "rb").read()


def test_ply_filter_rows_errors(lcgs, tmp_path):
    P = lcgs.read_gs_ply(TINY)["pos"].shape[0]
    out = str(tmp_path / "out.ply")

    def refused(status, path, keep):
        with pytest.raises(lcgs.LcgsError) as e:
            lcgs.ply_filter_rows(path, out, keep)
        assert e.value.status == status, (e.value.status, str(e.value))
        assert not os.path.exists(out)

    refused(FORMAT, TINY, np.ones(P - 1, np.uint8))  # a wrong row count
    ascii_ply = str(tmp_path / "ascii.ply")
    with open(ascii_ply, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n0 0\n")
    refused(FORMAT, ascii_ply, np.ones(1, np.uint8))
    refused(IO, str(tmp_path / "missing.ply"), np.ones(P, np.uint8))
    head, data = _payload(TINY)
    short = str(tmp_path / "short.ply")
    open(short, "wb").write(head + data[:-5])
    refused(FORMAT, short, np.ones(P, np.uint8))  # a truncated payload
    faces = str(tmp_path / "faces.ply")
    open(faces, "wb").write(head.replace(b"end_header\n", b"element face 0\nproperty list uchar int vertex_indices\nend_header\n") + data)
    refused(FORMAT, faces, np.ones(P, np.uint8))  # elements after `vertex`
    lib = lcgs.load_library()
    assert lib.lcgs_ply_filter_rows(None, out.encode(), 0, None) == INVALID_ARG
    assert lib.lcgs_ply_filter_rows(TINY.encode(), out.encode(), P, None) == INVALID_ARG
