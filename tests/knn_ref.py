"""NumPy restatement of lcgs_knn_mean_dist2 (include/lcgs_hip.h): the mean squared distance of every point to its three nearest
neighbours, brute force.

`mean_dist2_f32` is the yardstick the kernels must equal BIT FOR BIT: every difference, square and sum is a float32 array
operation in the contract's order, ((dx dx + dy dy) + dz dz), then ((a + b) + c) / 3.  `mean_dist2_f64` is the same in float64,
for sanity only.  Neither knows anything about the kernels' sort, chunks or pruning."""
import numpy as np


def valid_rows(pos):
    return np.isfinite(np.asarray(pos).reshape(-1, 3)).all(axis=1)


def _mean_dist2(pos, dtype, block=512):
    pos = np.ascontiguousarray(np.asarray(pos).reshape(-1, 3)).astype(dtype)
    n = pos.shape[0]
    out = np.zeros(n, dtype)
    ok = np.nonzero(valid_rows(pos))[0]
    p = pos[ok]
    v = p.shape[0]
    m = min(3, v - 1)
    if m <= 0:
        return out
    res = np.zeros(v, dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(0, v, block):
            q = p[a:a + block]
            dx = q[:, None, 0] - p[None, :, 0]
            dy = q[:, None, 1] - p[None, :, 1]
            dz = q[:, None, 2] - p[None, :, 2]
            xx = dx * dx
            yy = dy * dy
            zz = dz * dz
            d2 = xx + yy
            d2 = d2 + zz
            assert d2.dtype == dtype
            d2[np.arange(q.shape[0]), np.arange(a, a + q.shape[0])] = np.inf  # j != i: another INDEX
            # the m smallest values as a multiset (a point's own slot holds +inf, and m <= v - 1 values are never it -- unless a
            # true distance overflowed to +inf, which is then the same value)
            s = np.sort(np.partition(d2, m - 1, axis=1)[:, :m], axis=1)
            if m == 3:
                t = s[:, 0] + s[:, 1]
                t = t + s[:, 2]
                res[a:a + block] = t / dtype(3.0)
            elif m == 2:
                t = s[:, 0] + s[:, 1]
                res[a:a + block] = t / dtype(2.0)
            else:
                res[a:a + block] = s[:, 0]
    out[ok] = res
    return out


def mean_dist2_f32(pos):
    assert np.asarray(pos).dtype == np.float32
    return _mean_dist2(pos, np.float32)


def mean_dist2_f64(pos):
    return _mean_dist2(pos, np.float64)
