"""The 3DGS-MCMC restatement (tests/mcmc_ref.py) on the CPU: the relocation formulas' known cases, the sampler's exact integer
pieces and its distribution, the built-in normals' moments, the growth helper."""
import numpy as np

import mcmc_ref as ref

F32, F64 = np.float32, np.float64


def _logit(o):
    o = np.asarray(o, F64)
    return (np.log(o) - np.log1p(-o)).astype(F32)


# ------------------------------------------------------------------------------------------------------------ relocation values
def test_one_copy_is_the_identity():
    x = _logit(np.linspace(0.0051, 0.999, 400))
    log_c, raw_o, op, D = ref.relocated(x, np.zeros(x.size, int))  # count 0: n = 1
    o = 1.0 / (1.0 + np.exp(-x.astype(F64)))
    # o' = 1 - q carries q's rounding, a few 2^-53 ABSOLUTE: relative to o >= 0.0051 that is below 1e-13
    assert np.allclose(op, o, rtol=0, atol=4 * 2.0 ** -53) and np.abs(log_c).max() <= 1e-13
    assert np.array_equal(raw_o.astype(F32), x)  # the new raw opacity rounds back to the old one


def test_two_copies_agree_with_the_closed_form():
    x = np.concatenate([_logit(np.linspace(0.0051, 0.999, 400)), _logit([1 - 1e-7])])
    log_c, raw_o, op, D = ref.relocated(x, np.ones(x.size, int))
    xd = x.astype(F64)
    o, q = 1 / (1 + np.exp(-xd)), 1 / (1 + np.exp(xd))
    op2 = 1 - np.sqrt(q)
    D2 = 2 * op2 - op2 * op2 / np.sqrt(2.0)  # i = 1: o'; i = 2: o' - o'^2 / sqrt 2
    assert np.allclose(op, op2, rtol=1e-13) and np.allclose(D, D2, rtol=1e-13)
    assert np.allclose(log_c, np.log(o / D2), rtol=0, atol=1e-13)
    assert np.allclose((1 - op) ** 2, q, rtol=1e-12)  # two copies at o' leave the transmittance of one at o
    oh = np.clip(op2, F64(F32(0.005)), 1 - 2.0 ** -23)  # (min_opacity is a binary32 value)
    want = np.log(oh) - np.log1p(-oh)
    assert np.allclose(raw_o, want, rtol=0, atol=1e-12)


def test_scale_factor_falls_with_the_number_of_copies_and_stops_at_n_max():
    x = _logit([0.0051, 0.05, 0.5, 0.9, 0.999, 1 - 1e-7])
    prev = None
    for count in range(0, 51):
        log_c = ref.relocated(x, np.full(x.size, count))[0]
        assert np.isfinite(log_c).all()
        if prev is not None:
            assert (log_c < prev).all(), count
        prev = log_c
    at_max = ref.relocated(x, np.full(x.size, 50))
    for count in (51, 500, 2 ** 31):  # n = min(count + 1, 51)
        for a, b in zip(at_max, ref.relocated(x, np.full(x.size, count))):
            assert np.array_equal(a, b)
    assert np.array_equal(ref.relocated(x, np.full(x.size, 9), n_max=3)[0], ref.relocated(x, np.full(x.size, 2))[0])


def test_new_opacity_is_clamped_into_the_live_range():
    x = np.array([-5.29, 40.0, 800.0], F32)  # barely live -> o' below min_opacity; o = 1 in binary64 and beyond exp's range
    raw_o = ref.relocated(x, np.array([50, 0, 3]))[1]
    lo = np.log(F64(F32(0.005))) - np.log1p(-F64(F32(0.005)))
    hi = np.log(1 - 2.0 ** -23) - np.log1p(-(1 - 2.0 ** -23))
    assert np.isfinite(raw_o).all() and raw_o[0] == lo and raw_o[1] == hi and lo <= raw_o[2] <= hi


def test_liveness_rule_moves_a_clamped_opacity_by_at_most_one_step():
    """At min_opacity = 0.005 a binary32 step of the raw opacity moves its sigmoid by 5 ulp, the rounding of logit(min_opacity)
    and a last-place error of exp by at most 3.5: one step always suffices, so a relocated row's raw opacity stays within one
    binary32 ulp of the rounded binary64 value."""
    x = _logit(np.linspace(0.0051, 0.02, 300))  # sources whose o' falls below min_opacity for the larger counts
    for count in (1, 3, 50):
        raw_o = ref.relocated(x, np.full(x.size, count))[1]
        r, steps = ref.live_raw_opacity(raw_o)
        assert (ref.sigmoid32(r) > F32(0.005)).all() and steps.max() <= 1, steps.max()
        assert (np.abs(r.astype(F64) - raw_o.astype(F32).astype(F64)) <= np.spacing(np.abs(raw_o.astype(F32)))).all()
    # a sigmoid one ulp low everywhere (a worse exp than any in use) still needs one step only
    low = lambda v: np.nextafter(ref.sigmoid32(v), F32(0))
    r, steps = ref.live_raw_opacity(ref.relocated(x, np.full(x.size, 50))[1], sigmoid=low)
    assert (low(r) > F32(0.005)).all() and steps.max() <= 1


# ------------------------------------------------------------------------------------------------------------ the sampler
def test_weights_and_dead_rule():
    o = np.array([0.005, np.nextafter(F32(0.005), F32(1)), np.nan, 0.0, 0.5, 1.0, 0.75, 2.0 ** -24, 0.3], F32)
    w, dead = ref.weights(o, 0.005)
    assert dead.tolist() == [True, False, True, True, False, False, False, True, False]
    assert w.tolist() == [0, int(F64(o[1]) * 2 ** 24), 0, 0, 2 ** 23, 2 ** 24, 3 * 2 ** 22, 0, int(F64(o[8]) * 2 ** 24)]
    w2, dead2 = ref.weights(np.array([2.0 ** -24, 0.0], F32), 0.0)  # the smallest weight is 1
    assert w2.tolist() == [1, 0] and dead2.tolist() == [False, True]


def test_cdf_is_exact_in_u64_and_the_search_is_the_first_row_above():
    w = np.full(300, 2 ** 24, np.uint32)  # sums pass 2^32
    c = ref.cdf(w)
    assert c.dtype == np.uint64 and [int(v) for v in c[[0, 255, 256, 299]]] == [2 ** 24, 2 ** 32, 257 * 2 ** 24, 300 * 2 ** 24]
    assert ref.mulhi64(2 ** 64 - 1, 12345) == 12344 and ref.mulhi64(0, 12345) == 0
    assert ref.mulhi64(2 ** 63, 2 ** 40 + 1) == 2 ** 39
    c = np.array([0, 5, 5, 9], np.uint64)  # rows 0 and 2 have weight 0 and are never the first row ABOVE a t
    assert np.searchsorted(c, np.arange(9, dtype=np.uint64), side="right").tolist() == [1] * 5 + [3] * 4


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10"""
    kat = [((0, 0, 0, 0), 0, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, 0xFFFFFFFFFFFFFFFF, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), 0x299F31D0A4093822, (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = ref.philox4x32_10(*[np.array([v], np.uint64) for v in ctr], key)
        assert tuple(int(g[0]) for g in got) == want, (ctr, [hex(int(g[0])) for g in got])


def test_sampler_draws_live_rows_in_proportion_to_opacity():
    rng = np.random.default_rng(7)
    P, n = 5000, 200_000
    o = ref.sigmoid32(rng.normal(0, 2.5, P).astype(F32))
    w, dead = ref.weights(o, 0.005)
    assert 20 < dead.sum() < 300
    c = ref.cdf(w)
    assert int(c[-1]) == sum(int(x) for x in w)
    src = ref.draws(c, n, seed=1234, tag=ref.TAG_RELOCATE)
    assert src.min() >= 0 and src.max() < P and not dead[src].any()  # no draw lands on a dead row
    counts = np.bincount(src, minlength=P)
    live = np.nonzero(~dead)[0]
    order = live[np.argsort(o[live], kind="stable")]
    T, worst = float(int(c[-1])), 0.0
    for group in np.array_split(order, 16):  # 16 opacity-rank groups
        p = float(w[group].astype(np.float64).sum()) / T
        z = (counts[group].sum() - n * p) / np.sqrt(n * p * (1 - p))
        worst = max(worst, abs(z))
    print(f"[mcmc sampler] {int(dead.sum())} dead of {P}; 16 rank groups, max |z| = {worst:.2f}")
    assert worst <= 5.0, worst
    # another seed and another tag give other draws; the same give the same
    assert np.array_equal(src[:1000], ref.draws(c, 1000, seed=1234, tag=ref.TAG_RELOCATE))
    assert not np.array_equal(src[:1000], ref.draws(c, 1000, seed=1235, tag=ref.TAG_RELOCATE))
    assert not np.array_equal(src[:1000], ref.draws(c, 1000, seed=1234, tag=ref.TAG_ADD))


# ------------------------------------------------------------------------------------------------------------ the noise
def test_built_in_normals_have_standard_moments():
    P = 100_000
    z = ref.builtin_normals(P, seed=11, step=3).astype(F64)
    n_samples = P  # per component
    mean, var = z.mean(axis=0), z.var(axis=0)
    corr = np.array([(z[:, 0] * z[:, 1]).mean(), (z[:, 0] * z[:, 2]).mean(), (z[:, 1] * z[:, 2]).mean()])
    print(f"[mcmc normals] mean {mean}, var {var}, cross moments {corr}")
    assert (np.abs(mean) <= 5 / np.sqrt(n_samples)).all(), mean
    assert (np.abs(var - 1) <= 5 * np.sqrt(2 / n_samples)).all(), var
    assert (np.abs(corr) <= 5 / np.sqrt(n_samples)).all(), corr
    assert np.array_equal(z, ref.builtin_normals(P, seed=11, step=3).astype(F64))
    assert not np.array_equal(z[:100], ref.builtin_normals(100, seed=11, step=4).astype(F64))  # the step is part of the counter


def test_noise_model_gates_on_opacity():
    rng = np.random.default_rng(3)
    P = 64
    raw = {"pos": np.zeros((P, 3), F32), "scale": rng.normal(-4, 0.5, (P, 3)).astype(F32), "rotq": rng.normal(0, 1, (P, 4)).astype(F32),
           "opacity": _logit(np.linspace(0.001, 0.99, P))}
    eps = rng.normal(0, 1, (P, 3)).astype(F32)
    new64, g64 = ref.noise_step(raw, eps, lr_pos=1.6e-4, dtype=F64)
    new32, g32 = ref.noise_step(raw, eps, lr_pos=1.6e-4, dtype=F32)
    o = 1 / (1 + np.exp(-raw["opacity"].astype(F64)))
    assert (g64[o < 0.004] > 0.5).all() and (g64[o > 0.8] < 1e-32).all() and (np.diff(g64) < 0).all()
    R = ref.rotation(raw["rotq"].astype(F64), F64)
    S2 = np.exp(raw["scale"].astype(F64)) ** 2
    want = (80.0 * g64)[:, None] * np.einsum("nij,nj,nkj,nk->ni", R, S2, R, eps.astype(F64))
    assert np.allclose(new64, want, rtol=1e-6, atol=1e-300)
    assert np.allclose(new32, new64, rtol=1e-4, atol=1e-12)


def test_growth_helper(lcgs):
    f = lcgs.mcmc_num_new
    assert f(1000, 10_000) == 50 and f(1000, 1020) == 20 and f(1000, 1000) == 0 and f(1000, 900) == 0 and f(0, 10) == 0
    assert f(10, 100) == 0 and f(20, 100) == 1  # int(1.05 * 10) = 10
    n = 300
    for _ in range(40):
        n += f(n, 600)
    assert n == 600
