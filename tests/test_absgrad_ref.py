"""The reference of the AbsGS statistic (tests/absgrad_ref.py) held to account, without a GPU: the one-hot walks add up to the
oracle's own backward, the absolute sum dominates the signed one and lies under the walk's budget A, the f32 reference lies inside
the bound B the kernel is held to -- and the two statistics a wrong kernel would compute (the signed one, |sum_p g|; the per-tile
one, sum_tiles |sum_{p in tile} g|, i.e. the absolute value taken at the flush) lie OUTSIDE B on most rows, so tests/test_gpu_absgrad.py
cannot pass either of them.

Measured here (make_scene(default_rng(5), 300), camera at (0, 0, -4) looking at the origin):
  24 x 20, colour only:        signed outside B on 292 of 294 rows with a gradient; f32 worst diff / B 0.064; median B / abs 1.4e-3
  40 x 24, colour+depth+alpha: per-tile outside B on 288 of 292 rows, signed on 289; f32 worst diff / B 0.127; median B / abs 1.9e-3"""
import numpy as np
import pytest

import absgrad_ref as R
from gpu_util import U32, _oracles, cached

FRAMES = {"colour_24x20": (24, 20, dict(colour=True, depth=False, alpha=False)),
          "three_40x24": (40, 24, dict(colour=True, depth=True, alpha=True))}


def _ref(name):
    W, H, ch = FRAMES[name]

    def make():
        o32 = _oracles()[0]
        di, dd, da = R.gradients(W, H, 11, **ch)
        return R.reference(R.scene300(), o32.lookat(*R.POSE, width=W, height=H), di, dd, da, mode="z", bg=R.BG)

    return cached(("absgrad_ref", name), make)


@pytest.mark.parametrize("name", list(FRAMES))
def test_one_hot_walks_add_up_to_the_full_backward(name):
    """sum_p g(p, .) is the oracle's render_backward of the whole dL: to f64 rounding in the f64 build, to f32 rounding (counted by
    the walk's own budget A) in the f32 build"""
    ref = _ref(name)
    A = ref["A"]
    d64 = np.abs(ref["r64"]["sum"].astype(np.float64) - ref["r64"]["full"].astype(np.float64))
    assert (d64 <= 64 * 2.0 ** -53 * A).all(), float((d64 / np.maximum(A, 1e-300)).max())
    d32 = np.abs(ref["r32"]["sum"].astype(np.float64) - ref["r32"]["full"].astype(np.float64))
    assert (d32 <= 64 * U32 * A).all(), float((d32 / np.maximum(A, 1e-300)).max())
    assert (np.abs(ref["r64"]["full"]) > 0).any()


def test_the_shortcut_is_the_plain_one_hot_call_bit_for_bit():
    """a state whose n_contrib is zero outside p gives the same g(p, .) as the state as it is: a pixel with a zero dL adds exact zeros"""
    W, H, ch = FRAMES["three_40x24"]
    o32 = _oracles()[0]
    cam = o32.lookat(*R.POSE, width=W, height=H)
    scene = R.scene300()
    st = R.Classic.state(o32, scene, cam, 1.0, 3)
    walks = R._walks(o32, st, scene, cam, *R.gradients(W, H, 11, **ch), "z", R.BG, 1.0)
    drawn = np.argwhere(np.asarray(st["n_contrib"]).reshape(H, W) > 0)
    assert len(drawn) > 40
    pixels = [(int(x), int(y)) for y, x in drawn[::len(drawn) // 20]] + [(0, 0), (W - 1, H - 1)]  # (the corners: nothing drawn)
    assert len({(x // 16, y // 16) for x, y in pixels}) >= 3  # several tiles
    hit = 0
    for x, y in pixels:
        a = R.pixel_gradient(o32, st, W, H, walks, x, y, shortcut=True)
        b = R.pixel_gradient(o32, st, W, H, walks, x, y, shortcut=False)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (x, y)
        hit += int((a != 0).any())
    assert hit >= len(pixels) // 2, (hit, len(pixels))


@pytest.mark.parametrize("name", list(FRAMES))
def test_absolute_sum_dominates_the_signed_one_and_lies_under_the_budget(name):
    ref = _ref(name)
    assert (ref["abs64"] >= ref["signed64"]).all()
    assert (ref["abs64"] >= ref["tiles64"] * (1 - 1e-12)).all() and (ref["tiles64"] >= ref["signed64"] * (1 - 1e-12)).all()
    assert (ref["A"] >= ref["abs64"]).all()
    assert (ref["abs32"] >= np.abs(ref["r32"]["sum"].astype(np.float64)) * (1 - 1e-5)).all()


@pytest.mark.parametrize("name, wrong", [("colour_24x20", "signed64"), ("three_40x24", "signed64"), ("three_40x24", "tiles64")])
def test_a_wrong_kernel_cannot_pass(name, wrong):
    """the signed and the per-tile statistics lie outside B on at least half of the rows that have a gradient"""
    ref = _ref(name)
    rows = (ref["abs64"] > 0).any(axis=1)
    out = ((np.abs(ref[wrong] - ref["abs64"]) > ref["B"]).any(axis=1)) & rows
    print(f"[absgrad ref] {name}: {wrong} outside B on {int(out.sum())} of {int(rows.sum())} rows with a gradient")
    assert rows.sum() > 250 and out.sum() >= 0.5 * rows.sum()


@pytest.mark.parametrize("name", list(FRAMES))
def test_the_f32_reference_lies_inside_the_bound(name):
    ref = _ref(name)
    r = np.maximum(R.ratios(ref["abs32"], ref), R.ratios(ref["abs32c"], ref))
    rows = ref["abs64"] > 0
    tight = np.median(ref["B"][rows] / ref["abs64"][rows])
    print(f"[absgrad ref] {name}: f32 worst diff / B {r.max():.3f}; median B / abs {tight:.2e}")
    assert r.max() <= 1.0
    assert tight < 1e-2  # the bound is tight: a percent of the statistic would not pass
