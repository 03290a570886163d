"""The yardstick of the photometric loss pinned without a GPU (tests/photometric_ref.py): the autograd form and the closed
form agree, and the definition has the properties it should."""
import pytest
import torch

import photometric_ref as R

SIZES = [(37, 53), (16, 16), (7, 5), (1, 1)]  # (W, H)


def _pair(W, H, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(3, H, W, generator=g, dtype=torch.float64), torch.rand(3, H, W, generator=g, dtype=torch.float64)


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-300)


@pytest.mark.parametrize("lam", [0.0, 0.2, 1.0])
@pytest.mark.parametrize("W,H", SIZES)
def test_autograd_and_closed_form_agree(W, H, lam):
    x, y = _pair(W, H, 100 * W + H)
    loss_i, terms_i, grad_i = R.autograd(x, y, lam)
    loss_ii, terms_ii, grad_ii = R.combine(R.closed_form(x, y), lam)
    assert _rel(loss_ii, loss_i) <= 1e-12
    assert _rel(terms_ii, terms_i) <= 1e-12
    assert _rel(grad_ii, grad_i) <= 1e-12


@pytest.mark.parametrize("W,H", SIZES)
def test_an_image_against_itself(W, H):
    x, _ = _pair(W, H, 7)
    loss, terms, grad = R.autograd(x, x.clone(), 0.2)
    assert abs(terms[1].item() - 1.0) <= 1e-14 and terms[0].item() == 0.0 and abs(loss.item()) <= 1e-14
    # sign(0) = 0, and SSIM is at its maximum: the gradient vanishes up to the rounding of the cancelling terms
    assert grad.abs().max().item() <= 1e-12
    parts = R.closed_form(x, x.clone())
    assert abs(parts["ssim"].item() - 1.0) <= 1e-14 and parts["g_ssim"].abs().max().item() <= 1e-12


@pytest.mark.parametrize("W,H", SIZES)
def test_the_loss_is_symmetric(W, H):
    x, y = _pair(W, H, 11)
    a, ta, _ = R.autograd(x, y, 0.2)
    b, tb, _ = R.autograd(y, x, 0.2)
    assert _rel(a, b) <= 1e-14 and _rel(ta, tb) <= 1e-14


def test_the_window_sums_to_one():
    w = R.window()
    assert w.dtype == torch.float64 and w.numel() == 11
    assert abs(w.sum().item() - 1.0) <= 1e-15
    assert torch.equal(w, w.flip(0)) and w.argmax().item() == 5
