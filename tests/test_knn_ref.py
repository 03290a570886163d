"""The NumPy restatement of lcgs_knn_mean_dist2 (tests/knn_ref.py) against cases whose answer is known, and against itself."""
import numpy as np

from knn_ref import mean_dist2_f32, mean_dist2_f64


def test_integer_lattice_gives_exactly_one():
    g = np.arange(8, dtype=np.float32)
    pos = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    assert np.array_equal(mean_dist2_f32(pos), np.ones(512, np.float32))
    assert np.array_equal(mean_dist2_f64(pos), np.ones(512, np.float64))


def test_fewer_than_three_neighbours():
    two = np.array([[0, 0, 0], [1, 2, 2]], np.float32)
    assert np.array_equal(mean_dist2_f32(two), np.array([9, 9], np.float32))  # m = 1: a itself
    assert np.array_equal(mean_dist2_f32(two[:1]), np.zeros(1, np.float32))  # m = 0
    three = np.array([[0, 0, 0], [1, 0, 0], [0, 3, 0]], np.float32)
    assert np.array_equal(mean_dist2_f32(three), np.array([5, 5.5, 9.5], np.float32))  # m = 2: (a + b) / 2
    assert mean_dist2_f32(np.zeros((0, 3), np.float32)).shape == (0,)


def test_coincident_points_are_neighbours_at_distance_zero():
    pos = np.repeat(np.array([[1, 2, 3], [4, 5, 6]], np.float32), 4, axis=0)
    assert np.array_equal(mean_dist2_f32(pos), np.zeros(8, np.float32))


def test_invalid_rows_give_zero_and_are_nobodys_neighbour():
    rng = np.random.default_rng(0)
    pos = rng.normal(size=(50, 3)).astype(np.float32)
    bad = pos.copy()
    bad[[3, 17], 1] = np.nan
    bad[40, 0] = np.inf
    got = mean_dist2_f32(bad)
    keep = np.setdiff1d(np.arange(50), [3, 17, 40])
    assert np.array_equal(got[keep], mean_dist2_f32(pos[keep])) and not got[[3, 17, 40]].any()


def test_float32_agrees_with_float64():
    rng = np.random.default_rng(1)
    pos = rng.uniform(0, 1, (1500, 3)).astype(np.float32)
    a, b = mean_dist2_f32(pos), mean_dist2_f64(pos)
    assert a.dtype == np.float32 and b.dtype == np.float64 and (b > 0).all()
    assert np.abs(a - b).max() <= 1e-6 * b.max() and np.allclose(a, b, rtol=1e-6, atol=0)


def test_permuting_the_input_permutes_the_output_bit_for_bit():
    rng = np.random.default_rng(2)
    pos = rng.normal(size=(1200, 3)).astype(np.float32)
    perm = rng.permutation(1200)
    assert np.array_equal(mean_dist2_f32(pos[perm]), mean_dist2_f32(pos)[perm])
