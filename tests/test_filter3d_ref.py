"""The 3-D smoothing filter's restatement (tests/filter3d_ref.py) without a GPU: its binary32 form stays inside the bounds counted
for it against its binary64 form, apply + backward agree with torch float64 autograd of the same formulas, the tangent-plane
visibility rule is Mip-Splatting's pixel-space rule, the draws the GPU tests run leave few rows undecided, and the product of
ratios survives where the quotient of determinants underflows.  tests/test_gpu_filter3d.py holds the kernels to the same
restatement."""
import numpy as np
import pytest
import torch

import filter3d_ref as R

U = R.U


@pytest.fixture(scope="module")
def rows():
    return R.draw_rows(np.random.default_rng(2024), 200_000)


def _worst(err, scale):
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(scale > 0, err / scale, np.where(err > 0, np.inf, 0.0))
    return float(q.max())


def test_binary32_apply_and_backward_stay_inside_the_counted_bounds(rows):
    """scale_out 3 u, opacity_out 8 u, g_op' 8 u relative; g_s_k' 16 u (|first term| + |second term|), both terms in binary64
    (measured on this draw: 1.9 u, 4.4 u, 4.4 u and 6.9 u)"""
    scale, opacity, filt, gs, go = rows
    s32, o32 = R.apply(scale, opacity, filt)
    s64, o64 = R.apply(scale, opacity, filt, np.float64)
    assert s32.dtype == o32.dtype == np.float32 and np.isfinite(s64).all() and np.isfinite(o64).all()
    a, b = _worst(np.abs(s32 - s64), np.abs(s64)), _worst(np.abs(o32 - o64), np.abs(o64))
    gs32, go32 = R.backward(scale, opacity, filt, gs, go)
    gs64, go64, terms = R.backward(scale, opacity, filt, gs, go, np.float64, terms=True)
    on = filt != 0
    c, d = _worst(np.abs(go32 - go64), np.abs(go64)), _worst(np.abs(gs32 - gs64)[on], terms[on])
    print(f"[filter3d f32 vs f64] scale_out {a / U:.2f} u, opacity_out {b / U:.2f} u, g_op' {c / U:.2f} u, g_s' {d / U:.2f} u of the terms")
    assert a <= R.BOUND_SCALE and b <= R.BOUND_OPACITY and c <= R.BOUND_G_OPACITY and d <= R.BOUND_G_SCALE, (a / U, b / U, c / U, d / U)
    # the identity rows are the inputs' bits, in both directions
    off = ~on
    assert off.sum() >= 20_000
    assert np.array_equal(s32[off].view(np.uint32), scale[off].view(np.uint32)) and np.array_equal(o32[off].view(np.uint32), opacity[off].view(np.uint32))
    assert np.array_equal(gs32[off].view(np.uint32), gs[off].view(np.uint32)) and np.array_equal(go32[off].view(np.uint32), go[off].view(np.uint32))


def test_backward_is_the_gradient_of_apply(rows):
    """apply then backward, binary64, against torch float64 autograd of Mip-Splatting's formulas"""
    scale, opacity, filt, gs, go = (x[:5000] for x in rows)
    s = torch.tensor(scale, dtype=torch.float64, requires_grad=True)
    o = torch.tensor(opacity, dtype=torch.float64, requires_grad=True)
    f = torch.tensor(filt, dtype=torch.float64)
    f2 = (f * f)[:, None]
    s_f = torch.sqrt(s * s + f2)
    # (the ratio s^2 / (s^2 + f^2) written as 1 / (1 + f^2 / s^2): autograd's two paths through a quotient of products cancel,
    # to 1e-16 (s^2 + f^2) / f^2 of the term, where s >> f)
    o_f = o * torch.sqrt(torch.prod(1.0 / (1.0 + f2 / (s * s)), dim=1))
    s64, o64 = R.apply(scale, opacity, filt, np.float64)
    literal = o * torch.sqrt(torch.prod(s * s, dim=1) / torch.prod(s * s + f2, dim=1))  # get_opacity_with_3D_filter as written
    assert np.allclose(s_f.detach().numpy(), s64, rtol=1e-13, atol=0) and np.allclose(o_f.detach().numpy(), o64, rtol=1e-12, atol=0)
    assert np.allclose(literal.detach().numpy(), o64, rtol=1e-12, atol=0)
    (s_f * torch.tensor(gs, dtype=torch.float64)).sum().add((o_f * torch.tensor(go, dtype=torch.float64)).sum()).backward()
    gs64, go64, terms = R.backward(scale, opacity, filt, gs, go, np.float64, terms=True)
    assert np.allclose(o.grad.numpy(), go64, rtol=1e-12, atol=0)
    on = filt != 0
    assert (np.abs(s.grad.numpy() - gs64)[on] <= 1e-11 * terms[on]).all()
    assert np.allclose(s.grad.numpy()[~on], gs[~on].astype(np.float64), rtol=1e-14, atol=0)  # the identity rows


@pytest.mark.parametrize("P", R.ACC_SIZES)
def test_tangent_plane_rule_is_the_pixel_rule_and_few_rows_are_undecided(lcgs, P):
    """On the GPU tests' own draws: 1.3 tan(fov / 2) in the tangent plane is the 15 % pixel margin, evaluated in binary64, for every
    (row, view) not flagged undecided; and for every view count the GPU tests use the undecided rows are at most 1 % of the rows --
    checked HERE, on the restatement alone, so that the GPU test cannot hide a failure behind its undecided rows."""
    pos, cams, ref = R.accumulate_case(lcgs, P)
    pix = R.seen_in_pixels(lcgs, pos, cams)
    finite = np.isfinite(pos).all(axis=1)  # (an infinite coordinate: inf <= inf holds, the pixel is NaN; min_z stays +inf either way)
    ok = ref["undecided"] | (ref["seen"] == pix) | ~finite[:, None]
    assert ok.all(), (int((~ok).sum()), np.argwhere(~ok)[:5].tolist())
    for V in R.ACC_VIEWS:
        und = ref["undecided"][:, :V].any(axis=1)
        assert und.sum() <= 0.01 * P, (V, int(und.sum()))
    if P >= 255:  # the draw reaches every branch of the rule
        z, seen = ref["z"], ref["seen"]
        assert seen.any() and (z < 0).any() and ((z > 0) & (z <= 0.2)).any() and ((z > 0.2) & ~seen).any()
        assert np.isinf(ref["min_z"][[5, 17, 40]]).all()  # NaN / inf positions are never seen
        assert np.isfinite(ref["min_z"]).any() and np.isinf(R.min_z_of(ref, 0, 1)).any()
    # a prefix of the views is a prefix of the columns; two halves combine to the whole
    V = len(cams)
    assert np.array_equal(R.min_z_of(ref, 0, V), ref["min_z"])
    assert np.array_equal(np.minimum(R.min_z_of(ref, 0, 40), R.min_z_of(ref, 40, V)), ref["min_z"])
    assert ref["max_focal"] == max(R.view_constants(lcgs, c)[4] for c in cams)


def test_finalize_restatement():
    mz = np.array([np.inf, 2.0, 0.5, np.inf, 3.0], np.float32)
    f = R.finalize(mz, 100.0)
    c = np.float32(np.sqrt(0.2))
    assert f.dtype == np.float32 and np.array_equal(f, (np.array([3.0, 2.0, 0.5, 3.0, 3.0], np.float32) / np.float32(100.0)) * c)
    near = [abs(float(x) - 0.2 ** 0.5) for x in (np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(1)))]
    assert near[1] < near[0] and near[1] < near[2]  # the binary32 nearest to sqrt(0.2)
    assert np.array_equal(R.finalize(np.full(7, np.inf, np.float32), 100.0), np.zeros(7, np.float32))


def test_product_of_ratios_survives_where_the_determinants_underflow():
    """scales of 1e-8 with f = 1e-3: prod(s^2) = 1e-48 is 0 in binary32, the product of the three ratios 1e-30 is not"""
    scale = np.full((4, 3), 1e-8, np.float32)
    filt = np.full(4, 1e-3, np.float32)
    s_f, o_f = R.apply(scale, np.full(4, 0.5, np.float32), filt)
    _, o64 = R.apply(scale, np.full(4, 0.5, np.float32), filt, np.float64)
    assert (R.coef_by_determinants(scale, filt) == 0).all()
    assert np.isfinite(o_f).all() and (o_f > 0).all() and (np.abs(o_f - o64) <= R.BOUND_OPACITY * o64).all()
    assert (np.abs(s_f - 1e-3) <= 1e-9).all()
