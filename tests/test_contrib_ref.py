"""The premises of tests/contrib_ref.py on the CPU oracle alone: the crowd is a frame on which a per-splat reduction can go
wrong in every way the kernel has (rows listed but never blended, rows blended in several tiles, lists of several rounds), the
one-hot composition adds up to the alpha map, and pruning the rows no pixel blends changes no pixel."""
import numpy as np

import contrib_ref
import maps_ref
from gpu_util import BG, cached


def _crowd(oracle):
    return cached(("contrib", "crowd views"), lambda: contrib_ref.crowd_views(oracle))


def test_the_crowd_exercises_every_path_of_the_reduction(oracle):
    scene, W, H, views = _crowd(oracle)
    s = views[0][2]
    st = s["state"]
    P = scene["pos"].shape[0]
    blended, listed = s["pixels"] > 0, np.zeros(P, bool)
    listed[s["listed"]] = True
    lens = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    print(f"[contrib ref] crowd: {int(blended.sum())} rows blended of {int(listed.sum())} listed, {int((s['tiles'] >= 2).sum())} in two "
          f"or more tiles (up to {int(s['tiles'].max())}), longest list {int(lens.max())}")
    assert not (blended & ~listed).any()
    assert (listed & ~blended).sum() >= 400        # rows on a list that no pixel blends: they must stay untouched
    assert (s["tiles"] >= 2).sum() >= 300          # rows whose statistics meet across workgroups
    assert lens.max() > 1024                       # five rounds of 256 staged entries
    # every blended weight is positive and at most 0.99; the max and the count agree about which rows were blended
    assert ((s["weight_max"] > 0) == blended).all() and s["weight_max"].max() <= np.float32(0.99)
    assert (s["weight_sum"][blended] >= s["weight_max"][blended]).all()
    assert (s["weight_sum"] <= s["pixels"] * s["weight_max"].astype(np.float64)).all()


def test_the_weights_add_up_to_the_alpha_map(oracle):
    scene, W, H, views = _crowd(oracle)
    for pose, cam, s in views:
        alpha = maps_ref.forward(oracle, scene, cam)[1]
        assert np.abs(s["total"] - alpha.astype(np.float64)).max() <= 1e-6
        # ... and the frame the weights were taken from is the oracle's own
        assert np.array_equal(s["state"]["n_contrib"], oracle.render(scene, cam)["n_contrib"])


def test_accumulating_two_views():
    a = {"weight_sum": np.array([1.0, 0.0, 2.0]), "weight_max": np.array([0.5, 0.0, 0.9], np.float32),
         "pixels": np.array([3, 0, 4], np.uint32)}
    b = {"weight_sum": np.array([0.5, 0.0, 0.0]), "weight_max": np.array([0.7, 0.0, 0.0], np.float32),
         "pixels": np.array([1, 0, 0], np.uint32)}
    acc = contrib_ref.accumulate([a, b])
    assert acc["weight_sum"].tolist() == [1.5, 0.0, 2.0] and acc["weight_max"].tolist() == [np.float32(0.7), 0.0, np.float32(0.9)]
    assert acc["pixels"].tolist() == [4, 0, 4] and acc["views"].tolist() == [2, 0, 1]
    keep = contrib_ref.keep_predicate(acc, min_weight_max=np.float32(0.7), min_views=1)
    assert keep.tolist() == [True, False, True]  # >=: a minimum exactly on a row's value keeps the row
    assert contrib_ref.keep_predicate(acc).all()  # nothing enabled: everything is kept


def test_pruning_rows_no_pixel_blends_changes_no_pixel(oracle):
    """The end-to-end property, on the oracle alone: a row no pixel of any view blends changes no pixel's sequence, so the
    sub-scene renders the same images bit for bit.  (The one way such a row can matter is as the entry that saturates a pixel --
    it ends the walk without being blended; none of the crowd's dropped rows does, or the equality below would not hold.)"""
    scene, W, H, views = _crowd(oracle)
    acc = contrib_ref.accumulate([s for _, _, s in views])
    keep = contrib_ref.keep_predicate(acc, min_pixels=1)
    P = scene["pos"].shape[0]
    print(f"[contrib ref] crowd, two views: {int(keep.sum())} of {P} rows kept")
    assert 1000 <= keep.sum() < P and ((acc["views"] == 2).sum() > 0) and ((acc["views"] == 1).sum() > 0)
    sub = contrib_ref.sub_scene(scene, keep)
    for pose, cam, _ in views:
        full, pruned = oracle.render(scene, cam, bg=BG)["img"], oracle.render(sub, cam, bg=BG)["img"]
        assert np.array_equal(full, pruned)
