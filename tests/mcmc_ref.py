"""A NumPy / Python-int restatement of the 3DGS-MCMC block of include/lcgs_hip.h: weights, the u64 cdf, Philox4x32-10,
mulhi64, the search, the binary64 relocation values and the SGLD noise.  tests/test_mcmc_ref.py checks the restatement on the
CPU; tests/test_gpu_mcmc.py holds the kernels to it."""
import numpy as np

F32, F64, U64 = np.float32, np.float64, np.uint64
SCAN_TILE = 1024  # kScanTile (csrc/kernels/scan.hip): rows per workgroup of the u64 scan, and sums per pass of its middle step
TAG_RELOCATE, TAG_ADD, TAG_NOISE = 0x4D430001, 0x4D430002, 0x4D430003
N_MAX = 51
_MASK = U64(0xFFFFFFFF)


def sigmoid32(x):
    """the optimiser step's expression, 1 / (1 + exp(-x)), in binary32 (NumPy's exp: the kernels' may differ in the last place)"""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x))).astype(F32)


def weights(o, min_opacity=0.005):
    """(w uint32, dead bool) of binary32 opacities o: dead iff !(o > min_opacity); w = dead ? 0 : trunc(o * 2^24), exact"""
    o = np.asarray(o, F32)
    with np.errstate(invalid="ignore"):
        dead = ~(o > F32(min_opacity))
    scaled = np.where(dead, F32(0), o) * F32(16777216.0)  # a power of two: no rounding; below o = 1 / 2 fraction bits remain
    return scaled.astype(np.uint32), dead  # ... and are truncated here


def cdf(w):
    return np.cumsum(np.asarray(w).astype(U64), dtype=U64)


def philox4x32_10(c0, c1, c2, c3, seed):
    """Philox4x32-10 over arrays of counters -> four uint64 arrays holding 32-bit words"""
    c = [np.asarray(x, U64) & _MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c[0], U64(0xCD9E8D57) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ U64(k0), p1 & _MASK, (p0 >> U64(32)) ^ c[3] ^ U64(k1), p0 & _MASK]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def mulhi64(u, T):
    return (int(u) * int(T)) >> 64


def draws(cdf_, n, seed, tag):
    """src_j, j = 0 .. n - 1: the smallest i with cdf_i > mulhi64(u_j, T)"""
    T = int(cdf_[-1])
    assert T > 0
    j = np.arange(n, dtype=U64)
    c = philox4x32_10(j & _MASK, j >> U64(32), tag, 0, seed)
    u = c[0] | (c[1] << U64(32))
    t = np.array([mulhi64(x, T) for x in u.tolist()], dtype=U64)
    return np.searchsorted(cdf_, t, side="right").astype(np.int64)


def binomials():
    C = np.zeros((N_MAX, N_MAX), F64)
    for i in range(N_MAX):
        C[i, 0] = 1.0
        for k in range(1, i + 1):
            C[i, k] = C[i - 1, k - 1] + (C[i - 1, k] if k < i else 0.0)
    return C


_BINOM = binomials()


def relocated(x, count, n_max=N_MAX, min_opacity=0.005):
    """binary64 relocation values of sources with original raw opacity x (binary32) and `count` draws ->
    (log c, new raw opacity, o', D), all binary64 (the kernels round log c + raw scale and the raw opacity once to binary32)"""
    x = np.atleast_1d(np.asarray(x, F32)).astype(F64)
    n = np.minimum(np.atleast_1d(count).astype(np.int64), n_max - 1) + 1
    with np.errstate(over="ignore"):  # (exp overflows to inf beyond |x| = 709: o or q is then exactly 0, as on the device)
        o, q = 1.0 / (1.0 + np.exp(-x)), 1.0 / (1.0 + np.exp(x))
    op = 1.0 - q ** (1.0 / n)
    D = np.zeros_like(x)
    for i in range(1, int(n.max()) + 1):
        on, pw = n >= i, op.copy()
        for k in range(i):
            term = _BINOM[i - 1, k] * pw / np.sqrt(F64(k + 1))
            D = np.where(on, D - term if k & 1 else D + term, D)
            pw = pw * op
    log_c = np.log(o / D)
    oh = np.minimum(np.maximum(op, F64(F32(min_opacity))), 1.0 - 2.0 ** -23)
    return log_c, np.log(oh) - np.log1p(-oh), op, D


def live_raw_opacity(raw_o, min_opacity=0.005, sigmoid=sigmoid32):
    """the liveness rule: the binary32 rounding of a new raw opacity, moved up by binary32 steps (at most 64) while `sigmoid` of
    it is not > min_opacity -> (binary32 values, steps taken).  The kernels apply it with THEIR sigmoid."""
    r = np.atleast_1d(np.asarray(raw_o, F64)).astype(F32)
    steps = np.zeros(r.shape, np.int64)
    for _ in range(64):
        dead = ~(sigmoid(r) > F32(min_opacity))
        if not dead.any():
            break
        r = np.where(dead, np.nextafter(r, F32(np.inf)), r).astype(F32)
        steps += dead
    return r, steps


def rotation(q, dtype):
    """R[..., row, col] of stored (r, x, y, z) quaternions by the kernels' expressions (act_unit, then rot_from_quat)"""
    q = np.asarray(q, dtype)
    one, two = dtype(1), dtype(2)
    n2 = one / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    w, x, y, z = q[:, 0] * n2, q[:, 1] * n2, q[:, 2] * n2, q[:, 3] * n2
    R = np.empty((q.shape[0], 3, 3), dtype)
    R[:, 0, 0] = one - two * y * y - two * z * z
    R[:, 1, 0] = two * x * y + two * z * w
    R[:, 2, 0] = two * x * z - two * y * w
    R[:, 0, 1] = two * x * y - two * z * w
    R[:, 1, 1] = one - two * x * x - two * z * z
    R[:, 2, 1] = two * y * z + two * x * w
    R[:, 0, 2] = two * x * z + two * y * w
    R[:, 1, 2] = two * y * z - two * x * w
    R[:, 2, 2] = one - two * x * x - two * y * y
    return R


def noise_step(raw, eps, lr_pos, noise_lr=5e5, k=100.0, x0=0.995, dtype=F32):
    """pos + (noise_lr lr_pos g(o)) R S^2 R^T eps in `dtype`, operation by operation as k_mcmc_noise -> (new pos, gain g)"""
    one = dtype(1)
    gain = dtype(F32(noise_lr) * F32(lr_pos))  # formed in binary32 on the host
    x = np.asarray(raw["opacity"], F32).astype(dtype)
    with np.errstate(over="ignore"):
        o = one / (one + np.exp(-x))
        g = one / (one + np.exp(-dtype(F32(k)) * ((one - o) - dtype(F32(x0)))))
    a = gain * g
    s = np.exp(np.asarray(raw["scale"], F32).astype(dtype))
    R = rotation(np.asarray(raw["rotq"], F32).astype(dtype), dtype)
    e = np.asarray(eps, F32).astype(dtype)
    t = np.stack([(R[:, 0, j] * e[:, 0] + R[:, 1, j] * e[:, 1] + R[:, 2, j] * e[:, 2]) * (s[:, j] * s[:, j]) for j in range(3)], 1)
    d = np.stack([R[:, c, 0] * t[:, 0] + R[:, c, 1] * t[:, 1] + R[:, c, 2] * t[:, 2] for c in range(3)], 1)
    return np.asarray(raw["pos"], F32).astype(dtype) + a[:, None] * d, g


def unit_open(x):
    return ((np.asarray(x, U64) >> U64(8)).astype(F32) + F32(0.5)) * F32(1.0 / 16777216.0)


def builtin_normals(P, seed, step):
    """the built-in sampler's three normals per row (binary32 Box-Muller; libm's log / sin / cos, so not bit for bit the kernels')"""
    i = np.arange(P, dtype=U64)
    c = philox4x32_10(i & _MASK, i >> U64(32), TAG_NOISE, step, seed)
    two_pi = F32(6.28318530717958647692)
    r0, t0 = np.sqrt(F32(-2) * np.log(unit_open(c[0]))), two_pi * unit_open(c[1])
    r1, t1 = np.sqrt(F32(-2) * np.log(unit_open(c[2]))), two_pi * unit_open(c[3])
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], 1).astype(F32)
