"""The yardstick of the depth-prior losses pinned without a GPU (tests/depth_prior_ref.py): the closed form the kernels implement
against torch's float64 autograd of the definition, Pearson's invariance under an affine change of the prior, the planted fit,
one patch that covers the image against the image, and the cap on the L1 pixels whose sign binary32 does not decide."""
import pytest
import torch

import depth_prior_ref as R

WEIGHT, ALPHA_MIN = R.abi32(0.7), R.abi32(1e-3)
GIVEN = dict(align="given", scale=R.abi32(0.37), shift=R.abi32(1.9))
VARIANTS = {"pearson": dict(kind="pearson"), "l1_fit": dict(kind="l1"), "l1_given": dict(kind="l1", **GIVEN)}
NAMES = ("loss", "dL_ddepth", "dL_dalpha", "stats", "res")


def _agree(got, want, rel, tag, floor=0.0):
    """every array of `got` within rel x (the largest |value| of `want`'s array, or `floor` for the two gradients where that is
    larger)"""
    for name, g, w in zip(NAMES, got, want):
        assert torch.isfinite(g).all() and g.shape == w.shape, (tag, name)
        scale = max(w.abs().max().item(), floor if name.startswith("dL_") else 0.0)
        assert (g - w).abs().max().item() <= rel * scale, (tag, name, (g - w).abs().max().item(), scale)


def _pearson_term_scale(D, A, M, mask, weight, alpha_min):
    """the size of one of the two terms of Pearson's g_v, weight / (G n) (m - mu_m) / sqrt(..), carried to the maps.  Where
    r = 1 up to eps (class "affine") the terms cancel to rounding, and what the two forms can agree to is 1e-9 of a TERM, not
    of the difference."""
    v = D.double() / A.double().clamp_min(alpha_min)
    st = R._statistics(v, M.double(), mask, "fit", 0, (0, 0))
    g_v = weight / (st["nn"] * torch.sqrt((st["var_v"] + R.EPS) * (st["var_m"] + R.EPS)))[0] * st["cm"].abs().max()
    return (g_v * torch.maximum(1.0 / A.double().clamp_min(alpha_min), (D.double() / (A.double() ** 2)).abs()).max()).item()


# every class at the small sizes, the large frame on three
CASES = [(W, H, k) for W, H in ((1, 1), (5, 7), (37, 53)) for k in R.CLASSES] + [(320, 240, k) for k in ("noisy", "offset", "holes")]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("W,H,kind", CASES)
def test_closed_form_equals_autograd(W, H, kind, variant):
    D, A, M, mask = R.inputs(kind, W, H)
    kw = dict(weight=WEIGHT, alpha_min=ALPHA_MIN, **VARIANTS[variant])
    floor = _pearson_term_scale(D, A, M, mask, WEIGHT, ALPHA_MIN) if (kind, variant) == ("affine", "pearson") else 0.0
    _agree(R.closed_form(D, A, M, mask, **kw), R.autograd(D, A, M, mask, **kw), 1e-9, (kind, variant, W, H), floor)


@pytest.mark.parametrize("variant", ("pearson", "l1_fit"))
@pytest.mark.parametrize("patch,offset", [(32, (0, 0)), (32, (31, 31)), (64, (17, 40))])
def test_closed_form_equals_autograd_in_patch_mode(patch, offset, variant):
    for kind in ("noisy", "holes"):
        D, A, M, mask = R.inputs(kind, 75, 67)
        kw = dict(weight=WEIGHT, alpha_min=ALPHA_MIN, patch=patch, patch_offset=offset, **VARIANTS[variant])
        got, want = R.closed_form(D, A, M, mask, **kw), R.autograd(D, A, M, mask, **kw)
        _agree(got, want, 1e-9, (kind, variant, patch, offset))
        assert got[3][1].item() > 1 and got[3][2:].abs().max().item() == 0  # several groups; no fit reported


def test_pearson_is_invariant_to_an_affine_change_of_the_prior():
    D, A, M, mask = R.inputs("noisy", 37, 53)
    base = R.autograd(D, A, M, mask, weight=WEIGHT)[0].item()
    assert 0 < base < 2 * WEIGHT
    M64 = M.double()
    var_m = M64.var(unbiased=False).item()

    def tol(a):
        """eps is not scaled with the prior: r changes by the factor sqrt((var_m + eps) / (var_m + eps / a^2)), i.e. by less
        than eps / 2 (1 / var_m + 1 / (a^2 var_m)) of itself, |r| <= 1; the rest is binary64 rounding"""
        return WEIGHT * 0.5 * R.EPS * (1.0 / var_m + 1.0 / (a * a * var_m)) + 1e-12

    for a, b in ((3.0, -7.0), (0.01, 100.0)):
        assert abs(R.autograd(D, A, a * M64 + b, mask, weight=WEIGHT)[0].item() - base) <= tol(a)
    for a, b in ((-3.0, 2.0), (-0.5, 0.0)):
        assert abs(R.autograd(D, A, a * M64 + b, mask, weight=WEIGHT)[0].item() - (2 * WEIGHT - base)) <= tol(a)


def test_l1_fit_returns_the_planted_pair():
    for W, H in ((37, 53), (320, 240)):
        D, A, M, mask = R.inputs("affine", W, H)
        for fn in (R.autograd, R.closed_form):
            loss, _, _, stats, res = fn(D, A, M, mask, kind="l1", weight=WEIGHT)
            assert stats[:2].tolist() == [W * H, 1]
            assert abs(stats[2].item() - R.AFFINE_S) <= 1e-9 and abs(stats[3].item() - R.AFFINE_T) <= 1e-9
            assert res.abs().max().item() <= 1e-9 and loss.item() <= 1e-9


def test_one_patch_covering_the_image_equals_the_image():
    D, A, M, mask = R.inputs("holes", 29, 31)
    for variant in ("pearson", "l1_fit"):
        kw = dict(weight=WEIGHT, alpha_min=ALPHA_MIN, **VARIANTS[variant])
        whole, one = R.closed_form(D, A, M, mask, **kw), R.closed_form(D, A, M, mask, patch=32, patch_offset=(0, 0), **kw)
        for name, a, b in zip(NAMES, whole, one):
            if name == "stats":  # (patch mode reports no fit)
                assert torch.equal(a[:2], b[:2]) and b[2:].abs().max().item() == 0
            else:  # (the padded patch is summed in another order: binary64 rounding apart)
                assert (a - b).abs().max().item() <= 1e-12 * a.abs().max().item(), (variant, name)
                assert torch.equal(a == 0, b == 0), (variant, name)


def excluded(cls, D, A, M, mask, **kw):
    """(the L1 pixels tests/test_gpu_depth_prior.py leaves out of its element-wise comparison, the counted pixels, whether the
    fit is exact there)"""
    r64, r32 = R.autograd(D, A, M, mask, **kw), R.autograd(D, A, M, mask, dtype=torch.float32, **kw)
    counted = R.counted_pixels(A, M, mask, kw.get("align", "fit"), kw.get("patch", 0), kw.get("patch_offset", (0, 0)))
    assert int(counted.sum()) == int(r64[3][0].item())
    exact = R.fit_is_exact(cls, kw.get("align", "fit"), int(counted.sum()), kw.get("patch", 0))
    return R.sign_undecided(r64[4], r32[4], counted, exact), int(counted.sum()), exact


GPU_SIZES = [(1, 1), (2, 1), (5, 7), (37, 53), (31, 15), (32, 16), (33, 17), (320, 240)]  # tests/test_gpu_depth_prior.py: SIZES
GPU_PATCHES = [(33, 17, 32, (0, 0)), (33, 17, 32, (1, 1)), (33, 17, 32, (31, 31)), (320, 240, 64, (0, 0)), (320, 240, 64, (17, 40)),
               (320, 240, 128, (0, 0)), (29, 31, 32, (0, 0)), (100, 100, 128, (0, 0))]  # ... and PATCHES


@pytest.mark.parametrize("variant", ("l1_fit", "l1_given"))
@pytest.mark.parametrize("kind", R.CLASSES)
def test_few_l1_residuals_are_too_small_for_binary32_to_sign(kind, variant):
    """the GPU test may leave a pixel with |res| <= tau out of the element-wise comparison, at most 1 % of the counted pixels:
    the reference alone stays below that on every L1 input it uses (where the fit is exact nothing is compared element-wise)"""
    for W, H in GPU_SIZES:
        D, A, M, mask = R.inputs(kind, W, H)
        small, n_c, exact = excluded(kind, D, A, M, mask, weight=WEIGHT, alpha_min=ALPHA_MIN, **VARIANTS[variant])
        if (W, H) in ((37, 53), (320, 240)) and kind in ("noisy", "offset"):
            print(f"[depth prior, left out by the reference alone] {kind} {variant} {W}x{H}: {int(small.sum())} of {n_c} "
                  f"({100.0 * int(small.sum()) / n_c:.3f} %)")
        assert exact or int(small.sum()) <= 0.01 * n_c, (kind, variant, W, H, int(small.sum()), n_c)
        assert exact == (variant == "l1_fit" and (kind == "affine" or n_c == 2))


@pytest.mark.parametrize("kind", ("noisy", "holes"))
@pytest.mark.parametrize("W,H,patch,offset", GPU_PATCHES)
def test_few_l1_residuals_are_too_small_in_patch_mode(W, H, patch, offset, kind):
    D, A, M, mask = R.inputs(kind, W, H)
    small, n_c, exact = excluded(kind, D, A, M, mask, kind="l1", weight=WEIGHT, alpha_min=ALPHA_MIN, patch=patch, patch_offset=offset)
    assert not exact and int(small.sum()) <= 0.01 * n_c, (kind, W, H, patch, offset, int(small.sum()), n_c)


def test_float32_restatement_is_close_but_not_equal():
    """the bound of the GPU tests is not vacuous: E32 / S of the Pearson gradients lies far below 1 and above 0"""
    for kind in ("smooth", "noisy", "holes"):
        D, A, M, mask = R.inputs(kind, 37, 53)
        r64 = R.autograd(D, A, M, mask, weight=WEIGHT)
        r32 = R.autograd(D, A, M, mask, weight=WEIGHT, dtype=torch.float32)
        for a, b in zip(r64[1:3], r32[1:3]):
            rel = (a - b.double()).abs().max().item() / a.abs().max().item()
            assert 0 < rel < 1e-3, (kind, rel)
