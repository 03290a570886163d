"""Mip-Splatting's 3-D smoothing filter on the GPU (lcgs_filter3d_accumulate / _finalize / _apply / _backward) against its NumPy
restatement (tests/filter3d_ref.py): bit for bit where the restatement's binary32 operations are the kernels', inside the bounds
counted from the roundings against its binary64 form where the association is free.  The draws' undecided rows (comparisons
the host's tanf may tip) are capped in tests/test_filter3d_ref.py, on the restatement alone."""
import ctypes as C

import numpy as np
import pytest
import torch

import filter3d_ref as R
from conftest import make_scene
from gpu_util import DEV, dev

pytestmark = pytest.mark.gpu

KEYS = ("pos", "scale", "rotq", "sh", "opacity")
INF = np.float32(np.inf)


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def renderer(lcgs):
    return lcgs.Renderer(lcgs.Context(0))


def unaligned(a):
    """a device copy of `a` that starts 4 bytes past a 16-byte boundary: the kernels' scalar path"""
    flat = torch.empty(a.size + 1, device=DEV)
    t = flat[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


# ------------------------------------------------------------------------------------------------------------- accumulate
@pytest.mark.parametrize("P", R.ACC_SIZES)
def test_accumulate_is_the_restatement_bit_for_bit(lcgs, renderer, P):
    pos, cams, ref = R.accumulate_case(lcgs, P)
    d_pos = dev(pos)
    last = None
    for V in R.ACC_VIEWS:
        mz = torch.full((P,), float("inf"), device=DEV)
        focal = renderer.filter3d_accumulate(d_pos, cams[:V], mz)
        got = mz.cpu().numpy()
        want, und = R.min_z_of(ref, 0, V), ref["undecided"][:, :V]
        decided = ~und.any(axis=1)
        assert np.array_equal(bits(got)[decided], bits(want)[decided]), (V, int((bits(got) != bits(want))[decided].sum()))
        for i in np.nonzero(~decided)[0]:  # one of the values the undecided views allow
            z, sure = ref["z"][i, :V], ref["seen"][i, :V] & ~und[i]
            base = z[sure].min() if sure.any() else INF
            assert got[i] == base or any(got[i] == z[k] and z[k] < base for k in np.nonzero(und[i])[0]), (V, i, got[i], base)
        want_focal = max([float(R.view_constants(lcgs, c)[4]) for c in cams[:V]], default=0.0)
        assert abs(focal - want_focal) <= 2 * R.U * want_focal, (V, focal, want_focal)
        if V == 0:
            assert focal == 0.0 and np.isinf(got).all()
        if P >= 63:
            assert np.isinf(got[[5, 17, 40]]).all() and (got[[5, 17, 40]] > 0).all()  # NaN / inf positions are never seen
        last = got
    # the views split between two calls (inside a chunk, and not at its edge), the focal carried over: the same bits
    V = R.ACC_VIEWS[-1]
    mz = torch.full((P,), float("inf"), device=DEV)
    f1 = renderer.filter3d_accumulate(d_pos, cams[:40], mz)
    f2 = renderer.filter3d_accumulate(d_pos, cams[40:V], mz, f1)
    assert same_bits(mz, last) and f2 == focal >= f1 > 0
    # ... and arrays that are not 16-byte aligned
    mz_u = unaligned(np.full(P, INF, np.float32))
    renderer.filter3d_accumulate(unaligned(pos), cams, mz_u)
    assert same_bits(mz_u, last)


# --------------------------------------------------------------------------------------------------------------- finalize
def _min_z_case(kind, P):
    rng = np.random.default_rng(P)
    z = rng.uniform(0.21, 30.0, P).astype(np.float32)
    if kind == "none":
        z[:] = INF
    elif kind == "last":
        z[:-1] = INF
    elif kind == "mix":
        z[rng.random(P) < 0.4] = INF
        z[rng.random(P) < 0.01] = np.nan  # (not a value accumulate leaves; not finite: treated like +inf)
        z[-1] = INF
    return z


@pytest.mark.parametrize("kind,P", [("all", 70_001), ("none", 257), ("none", 70_001), ("last", 70_001), ("mix", 65), ("mix", 70_001),
                                    ("all", 1), ("none", 1)])
def test_finalize_is_the_restatement_bit_for_bit(renderer, kind, P):
    z = _min_z_case(kind, P)
    want = R.finalize(z, 1234.5)
    for d_z in (dev(z), unaligned(z)):
        filt = torch.full((P,), 7.0, device=DEV)
        renderer.filter3d_finalize(d_z, 1234.5, filt)
        assert same_bits(filt, want)
    assert (want == 0).all() == (kind == "none")
    if kind == "last":
        assert (want == want[-1]).all() and want[-1] > 0


# ------------------------------------------------------------------------------------------------------------------ apply
def _rows(P):
    scale, opacity, filt, gs, go = R.draw_rows(np.random.default_rng(100 + P), P)
    if P == 1:
        filt[0] = np.float32(0.013)  # (row 0 of the draw is an identity row)
    if P >= 65:  # identity rows whose scales are NaN, zero and negative: copied as they are
        scale[0], scale[10], scale[20, 1] = np.nan, 0.0, -0.5
        opacity[10] = np.nan
    return scale, opacity, filt, gs, go


@pytest.mark.parametrize("P", [1, 65, 70_001])
def test_apply_is_the_restatement_bit_for_bit_and_inside_the_bounds(renderer, P):
    scale, opacity, filt, _, _ = _rows(P)
    s32, o32 = R.apply(scale, opacity, filt)
    s64, o64 = R.apply(scale, opacity, filt, np.float64)
    for put in (dev, unaligned):
        s_out, o_out = torch.full((P, 3), 7.0, device=DEV), torch.full((P,), 7.0, device=DEV)
        renderer.filter3d_apply(put(scale), put(opacity), put(filt), s_out, o_out)
        assert same_bits(s_out, s32) and same_bits(o_out, o32)
    ident = filt == 0
    assert same_bits(s_out[torch.from_numpy(ident).to(DEV)], scale[ident]) and same_bits(o_out[torch.from_numpy(ident).to(DEV)], opacity[ident])
    ok = ~ident
    gs, go = s_out.cpu().numpy().astype(np.float64), o_out.cpu().numpy().astype(np.float64)
    assert (np.abs(gs - s64)[ok] <= R.BOUND_SCALE * np.abs(s64)[ok]).all() and (np.abs(go - o64)[ok] <= R.BOUND_OPACITY * np.abs(o64)[ok]).all()


def test_second_apply_into_a_bound_scene_drops_its_derived_rows(lcgs):
    """A context renders the arrays apply writes, with rows derived from them (declare_static); a second apply with another filter
    drops those rows (scene_arrays_written): the next frame is the new values' frame, and nothing derived is stale."""
    rng = np.random.default_rng(5)
    P, W, H = 20_000, 160, 120
    scene = make_scene(rng, P)
    d = {k: dev(scene[k]) for k in KEYS}
    cam = lcgs.get_lookat_cam([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1], width=W, height=H)
    r = lcgs.Renderer(lcgs.Context(0))
    s_f, o_f = torch.empty_like(d["scale"]), torch.empty_like(d["opacity"])
    r.filter3d_apply(d["scale"], d["opacity"], dev(np.full(P, 1e-3, np.float32)), s_f, o_f)
    r.bind_scene(d["pos"], s_f, d["rotq"], d["sh"], o_f)
    r.declare_static(d["pos"], s_f, d["rotq"])
    first = torch.zeros(3, H, W, device=DEV)
    assert r.forward(cam, first, sync=True) > 0 and r.verify_derived() == 0
    r.filter3d_apply(d["scale"], d["opacity"], dev(np.full(P, 0.05, np.float32)), s_f, o_f)
    r.ctx.synchronize()
    assert r.verify_derived() == 0
    fresh = lcgs.Renderer(lcgs.Context(0))
    s2, o2 = s_f.clone(), o_f.clone()
    fresh.bind_scene(d["pos"], s2, d["rotq"], d["sh"], o2)
    a, b = torch.zeros(3, H, W, device=DEV), torch.zeros(3, H, W, device=DEV)
    assert r.forward(cam, a, sync=True) == fresh.forward(cam, b, sync=True) > 0
    assert torch.equal(a, b) and not torch.equal(a, first)
    assert r.verify_derived() == 0


# --------------------------------------------------------------------------------------------------------------- backward
def _inside_backward_bounds(got_s, got_o, scale, opacity, filt, gs, go):
    gs64, go64, terms = R.backward(scale, opacity, filt, gs, go, np.float64, terms=True)
    on = filt != 0
    es, eo = np.abs(got_s.astype(np.float64) - gs64), np.abs(got_o.astype(np.float64) - go64)
    print(f"[filter3d backward vs f64] worst g_s' {np.max((es[on] / terms[on]), initial=0) / R.U:.2f} u of the terms, "
          f"g_op' {np.max(eo[on] / np.abs(go64[on]), initial=0) / R.U:.2f} u")
    assert (es[on] <= R.BOUND_G_SCALE * terms[on]).all() and (eo[on] <= R.BOUND_G_OPACITY * np.abs(go64[on])).all()
    return on


@pytest.mark.parametrize("P", [1, 65, 70_001])
def test_dense_backward_is_inside_the_bounds(renderer, P):
    scale, opacity, filt, gs, go = R.draw_rows(np.random.default_rng(100 + P), P)
    if P == 1:
        filt[0] = np.float32(0.013)
    for put in (dev, unaligned):
        d_gs, d_go = put(gs), put(go)
        renderer.filter3d_backward(put(scale), put(opacity), put(filt), d_gs, d_go)
        got_s, got_o = d_gs.cpu().numpy(), d_go.cpu().numpy()
        on = _inside_backward_bounds(got_s, got_o, scale, opacity, filt, gs, go)
        assert same_bits(got_s[~on], gs[~on]) and same_bits(got_o[~on], go[~on])  # identity rows: untouched


class SmallFrame:
    """300 splats in a 64 x 64 view, every fifth far off the screen, every seventh with the identity filter.  Each kept splat
    touches at most two tiles of the filtered frame, so that every sum the render-backward forms across tiles has at most two
    addends and its bits do not depend on the order the tiles finish in."""

    P, W, H = 300, 64, 64
    POSE = ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1])

    def __init__(self, lcgs, oracle):
        rng = np.random.default_rng(77)
        cand = make_scene(rng, 3000, log_scale=(-4.6, 0.4))
        cand["pos"][::5] += 50.0
        filt = np.exp(rng.normal(-4.5, 0.6, 3000)).astype(np.float32)
        filt[::7] = 0.0
        s_f, _ = R.apply(cand["scale"], cand["opacity"], filt)
        m2, depth, cov = oracle.project(cand["pos"], s_f, cand["rotq"], oracle.lookat(*self.POSE, width=self.W, height=self.H))
        keep = np.nonzero(oracle.allocate_tiles(self.W, self.H, depth, m2, cov)[2] <= 2)[0][:self.P]
        assert keep.size == self.P
        self.scene = {k: np.ascontiguousarray(cand[k][keep]) for k in KEYS}
        self.filt = np.ascontiguousarray(filt[keep])
        assert (self.filt == 0).sum() >= 20 and (self.scene["pos"][:, 0] > 40).sum() >= 30
        self.cam = lcgs.get_lookat_cam(*self.POSE, width=self.W, height=self.H)
        self.dL = np.random.default_rng(3).normal(size=(3, self.H, self.W)).astype(np.float32)


@pytest.fixture(scope="module")
def small(lcgs, oracle):
    return SmallFrame(lcgs, oracle)


def test_compact_backward_follows_the_frames_rows(lcgs, small):
    """rows and count straight from lcgs_visible_rows of a keep_state frame of the filtered scene (device addresses, the count
    read on the device)"""
    P, sc = small.P, small.scene
    r = lcgs.Renderer(lcgs.Context(0))
    d = {k: dev(sc[k]) for k in KEYS}
    d_filt = dev(small.filt)
    s_f, o_f = torch.empty_like(d["scale"]), torch.empty_like(d["opacity"])
    r.filter3d_apply(d["scale"], d["opacity"], d_filt, s_f, o_f)
    r.bind_scene(d["pos"], s_f, d["rotq"], d["sh"], o_f)
    n = r.forward(small.cam, torch.zeros(3, small.H, small.W, device=DEV), keep_state=True, sync=True)
    rows = r.visible_rows().cpu().numpy().astype(np.int64)
    V = rows.size
    assert n > 0 and 30 <= V < P and (small.filt[rows] == 0).any() and (small.filt[rows] != 0).any()
    rows_addr, count_addr = C.c_void_p(), C.c_void_p()
    assert lcgs.load_library().lcgs_visible_rows(r.ctx._h, C.byref(rows_addr), C.byref(count_addr)) == 0
    rng = np.random.default_rng(9)
    gs, go = rng.normal(0, 1, (P, 3)).astype(np.float32), rng.normal(0, 1, P).astype(np.float32)
    d_gs, d_go = dev(gs), dev(go)
    r.filter3d_backward(d["scale"], d["opacity"], d_filt, d_gs, d_go, rows=rows_addr.value, count=count_addr.value)
    got_s, got_o = d_gs.cpu().numpy(), d_go.cpu().numpy()
    on = _inside_backward_bounds(got_s[:V], got_o[:V], sc["scale"][rows], sc["opacity"][rows], small.filt[rows], gs[:V], go[:V])
    assert on.any() and not same_bits(got_s[:V][on], gs[:V][on])
    assert same_bits(got_s[:V][~on], gs[:V][~on]) and same_bits(got_o[:V][~on], go[:V][~on])  # identity rows
    assert same_bits(got_s[V:], gs[V:]) and same_bits(got_o[V:], go[V:])                      # rows beyond the count


def test_autograd_composition_is_backward_then_filter_backward(lcgs, small):
    """filter3d_autograd in front of render_autograd: the gradients of the unfiltered scale and opacity are, bit for bit,
    Renderer.backward of the filtered frame followed by filter3d_backward by hand"""
    sc = small.scene
    r = lcgs.Renderer(lcgs.Context(0))
    leaves = {k: dev(sc[k]).requires_grad_(True) for k in KEYS}
    d_filt, dL = dev(small.filt), dev(small.dL)
    s_f, o_f = lcgs.filter3d_autograd(r, leaves["scale"], leaves["opacity"], d_filt)
    img = lcgs.render_autograd(r, small.cam, leaves["pos"], s_f, leaves["rotq"], leaves["sh"], o_f)
    (img * dL).sum().backward()
    torch.cuda.synchronize()
    # by hand, on another context
    h = lcgs.Renderer(lcgs.Context(0))
    d = {k: dev(sc[k]) for k in KEYS}
    hs, ho = torch.empty_like(d["scale"]), torch.empty_like(d["opacity"])
    h.filter3d_apply(d["scale"], d["opacity"], d_filt, hs, ho)
    assert same_bits(hs, s_f) and same_bits(ho, o_f)
    h.bind_scene(d["pos"], hs, d["rotq"], d["sh"], ho)
    himg = torch.zeros(3, small.H, small.W, device=DEV)
    assert h.forward(small.cam, himg, keep_state=True, sync=True) > 0 and torch.equal(himg, img.detach())
    g = {k: torch.zeros_like(d[k]) for k in KEYS}
    h.backward(dL, *[g[k] for k in KEYS])
    h.filter3d_backward(d["scale"], d["opacity"], d_filt, g["scale"], g["opacity"])
    h.ctx.synchronize()
    for k in KEYS:
        assert same_bits(leaves[k].grad, g[k]), k
    assert float(leaves["scale"].grad.abs().max()) > 0 and float(leaves["opacity"].grad.abs().max()) > 0
