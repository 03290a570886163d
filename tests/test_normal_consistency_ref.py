"""The yardstick of the normal-consistency loss pinned without a GPU (tests/normal_consistency_ref.py): the closed form the
kernel implements against torch's float64 autograd of the definition on every input class, the sign and axis conventions on
planes whose normal is known, and the clamp's one-sided gradient at alpha = alpha_min."""
import math

import numpy as np
import pytest
import torch

import normal_consistency_ref as R

SIZES = [(3, 3), (4, 3), (5, 7), (37, 53), (64, 64)]  # (W, H)
WEIGHT, ALPHA_MIN = R.abi32(0.05), R.abi32(1e-3)


@pytest.mark.parametrize("kind", R.CLASSES)
@pytest.mark.parametrize("W,H", SIZES)
def test_closed_form_equals_autograd(W, H, kind):
    cam = R.camera(W, H)
    D, A, N = R.inputs(kind, W, H)
    want = R.autograd(D, A, N, cam, WEIGHT, ALPHA_MIN)
    got = R.closed_form(D, A, N, cam, WEIGHT, ALPHA_MIN)
    for name, g, w in zip(("loss", "dL_ddepth", "dL_dalpha", "dL_dnormal"), got, want):
        assert torch.isfinite(g).all() and g.shape == w.shape, name
        scale = w.abs().max().item()
        assert (g - w).abs().max().item() <= 1e-12 * scale, (name, kind, (g - w).abs().max().item(), scale)
    if kind == "degenerate":
        assert bool((got[1] == 0).all()) and bool((want[1] == 0).all())
    elif min(W, H) > 4:  # (the one interior pixel of 3 x 3 "holes" is the hole with alpha = 0, whose rendered normal is 0)
        assert all(x.abs().max().item() > 0 for x in got[1:])
    # dL/dnormal is zero on the frame's rim; dL/ddepth and dL/dalpha reach the rim through its interior neighbours, except at
    # the corners
    rim = torch.ones(H, W, dtype=torch.bool)
    rim[1:-1, 1:-1] = False
    assert bool((got[3][:, rim] == 0).all())
    corners = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    assert all(got[1][y, x] == 0 and got[2][y, x] == 0 for y, x in corners)  # no interior pixel has a corner for a neighbour


def _plane(cam, nn, d=3.0, alpha=0.7):
    """the maps of the plane nn . P = d seen through cam, with the rendered normal nn alpha"""
    xs, ys = R._rays(cam, torch.float64)
    z = d / (nn[0] * xs[None, :] + nn[1] * ys[:, None] + nn[2])
    A = torch.full_like(z, alpha)
    N = torch.tensor(nn, dtype=torch.float64).view(3, 1, 1) * A
    return z * A, A, N


def test_fronto_parallel_plane_has_loss_zero_and_normal_minus_z():
    cam = R.camera(37, 23)
    D, A, N = _plane(cam, (0.0, 0.0, -1.0), d=-3.0)
    nt = R.surface_normal(D, A, cam, ALPHA_MIN)[4]
    want = torch.tensor([0.0, 0.0, -1.0], dtype=torch.float64).view(3, 1, 1).expand_as(nt)
    assert (nt - want).abs().max().item() <= 1e-12
    loss = R.autograd(D, A, N, cam, 1.0, ALPHA_MIN)[0]
    assert abs(loss.item()) <= 1e-12
    assert abs(R.closed_form(D, A, N, cam, 1.0, ALPHA_MIN)[0].item()) <= 1e-12


@pytest.mark.parametrize("axis", ("x", "y"))
@pytest.mark.parametrize("angle", (0.3, -0.45))
def test_tilted_plane_gives_the_analytic_normal(axis, angle):
    """a plane tilted about the view x axis has the normal (0, sin t, -cos t), about y (sin t, 0, -cos t): the surface normal comes
    out as that vector, facing the camera (negative z) -- which pins rx to the column index, ry to the row index and the sign"""
    cam = R.camera(41, 29)
    s, c = math.sin(angle), math.cos(angle)
    nn = (0.0, s, -c) if axis == "x" else (s, 0.0, -c)
    D, A, N = _plane(cam, nn, d=-3.0)
    assert bool((D > 0).all())  # in front of the camera
    nt = R.surface_normal(D, A, cam, ALPHA_MIN)[4]
    want = torch.tensor(nn, dtype=torch.float64).view(3, 1, 1).expand_as(nt)
    assert (nt - want).abs().max().item() <= 1e-10, (nt - want).abs().max().item()
    assert abs(R.closed_form(D, A, N, cam, 1.0, ALPHA_MIN)[0].item()) <= 1e-10  # the rendered normal agrees: no loss


def test_clamp_gradient_is_one_sided_at_alpha_min():
    W, H = 9, 7
    cam = R.camera(W, H)
    D, A, N = R.inputs("noisy", W, H)
    y, x = 3, 4
    D[y, x] = 3.2 * ALPHA_MIN  # (a surface point at z = 3.2 seen through alpha = alpha_min)
    c = WEIGHT / ((W - 2) * (H - 2))
    for a, passes in ((np.float32(ALPHA_MIN), True), (np.nextafter(np.float32(ALPHA_MIN), np.float32(0)), False)):
        A2 = A.clone()
        A2[y, x] = float(a)
        for fn in (R.autograd, R.closed_form):
            _, g_d, g_a, _ = fn(D, A2, N, cam, WEIGHT, ALPHA_MIN)
            through_z = -g_d[y, x].item() * float(D[y, x]) / ALPHA_MIN  # -g_z D / alpha^2 at alpha = alpha_min
            assert abs(through_z) > 1e3 * c  # (not a pixel where the question is moot)
            if passes:
                assert abs(g_a[y, x].item() - (c + through_z)) <= 1e-12 * abs(through_z), fn.__name__
            else:
                assert g_a[y, x].item() == c, fn.__name__


def test_float32_restatement_is_close_but_not_equal():
    """the bound of the GPU tests is not vacuous: E32 / S of the gradients lies far below 1 and above 0 on the first three classes"""
    for kind in ("smooth", "noisy", "holes"):
        cam = R.camera(37, 53)
        D, A, N = R.inputs(kind, 37, 53)
        r64 = R.autograd(D, A, N, cam, WEIGHT, ALPHA_MIN)
        r32 = R.autograd(D, A, N, cam, WEIGHT, ALPHA_MIN, torch.float32)
        for a, b in zip(r64[1:], r32[1:]):
            rel = (a - b.double()).abs().max().item() / a.abs().max().item()
            assert 0 < rel < 1e-3, (kind, rel)
