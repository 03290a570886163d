"""Helpers shared by the `-m gpu` parity tests (torch is only the owner of device memory here)."""
import numpy as np
import torch

DEV = "cuda:0"


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


def upload_scene(scene):
    return {k: dev(scene[k]) for k in ("pos", "scale", "rotq", "sh", "opacity")}


def device_bytes_lost(once, rounds=4):
    """Free device memory before minus after `rounds` calls of once(), following one warm-up call (the first use pays for
    one-off allocations of the runtime): what create / use / close rounds did not give back."""
    once()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(rounds):
        once()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return free0 - torch.cuda.mem_get_info()[0]


def assert_image_parity(gpu_img, orc, **_legacy):
    """The HIP frame must equal the oracle's BIT FOR BIT -- every pixel, no tolerance, no exempt pixels.

    BASELINE's bar is 1e-4 per-pixel L-inf; until round 3 this helper held every pixel to it except those whose
    oracle evaluation came within 1e-5 of a hard threshold (alpha < 1/255, T < 1e-4), because v_exp_f32 and libm's
    expf differ by an ulp or two and an ulp flips a threshold.  The blend's exp is now one defined sequence of binary32
    operations on both sides (gs_math.hpp::blend_exp = oracle/lcgs_oracle.c::orc_blend_exp), every other operation
    already was, so the comparison is exact equality (NaN pixels, where a test feeds non-finite inputs, must be NaN
    on both sides).  Returns (max |diff|, differing pixels) = (0.0, 0) for callers that report them."""
    ref = orc["img"]
    assert gpu_img.shape == ref.shape and gpu_img.dtype == ref.dtype == np.float32
    same = (gpu_img.view(np.uint32) == ref.view(np.uint32)) | ((gpu_img == ref))  # +0 / -0 compare equal
    both_nan = np.isnan(gpu_img) & np.isnan(ref)
    ok = same | both_nan
    if not ok.all():
        bad = ~ok.all(axis=0)
        with np.errstate(invalid="ignore"):
            diff = np.abs(gpu_img.astype(np.float64) - ref.astype(np.float64)).max(axis=0)
        amb = orc.get("ambig")
        n_amb = int((bad & amb.astype(bool)).sum()) if amb is not None else -1
        ys, xs = np.nonzero(bad)
        raise AssertionError(f"{int(bad.sum())} of {bad.size} pixels differ from the oracle (max |diff| "
                             f"{np.nanmax(diff[bad]):.3e}; {n_amb} of them threshold-ambiguous); first at "
                             f"(x={xs[0]}, y={ys[0]}): gpu {gpu_img[:, ys[0], xs[0]]} oracle {ref[:, ys[0], xs[0]]}")
    print(f"[parity] {ref.shape[2]}x{ref.shape[1]}: bit-identical to the oracle")
    return 0.0, 0


LIBM_AMBIG_EPS = 1e-5


def assert_parity_vs_libm_expf(gpu_img, oracle, scene, ocam, **render_kw):
    """The HIP frame against the oracle evaluated with a STANDARD exp (libm's expf) in the blend -- the footing the
    reference stands on (gs_tile_splatter/shader.cpp:256-265 says `exp(power)`; BASELINE's bar is 1e-4 per-pixel L-inf).
    The kernels' exp is a defined <= 2.73-ulp polynomial (gs_math.hpp::blend_exp), so against libm the frame moves by a few
    1e-7 everywhere and by up to ~1e-2 where an ulp flips a hard threshold (`alpha < 1/255` skips an entry, `T < 1e-4` ends
    the pixel).  Asserted: (i) pixels beyond 1e-4 are at most 1e-5 of the frame, (ii) EVERY one of them is flagged
    threshold-ambiguous by the libm oracle itself (some alpha or test_T within LIBM_AMBIG_EPS relative of its threshold --
    1e-5, not a few ulp, because T carries the relative error of every earlier (1 - alpha) factor, each amplified by up to
    1 / (1 - 0.99)), (iii) every unflagged pixel is within 2e-6.
    Returns {pixels_over_1e-4, max_abs_diff, all_flagged, ambiguous_pixels, max_unflagged}."""
    oracle.set_blend_exp(True)
    try:
        ref = oracle.render(scene, ocam, ambig_eps=LIBM_AMBIG_EPS, **render_kw)
    finally:
        oracle.set_blend_exp(False)
    st = libm_parity_stats(gpu_img, ref)
    n = gpu_img.shape[1] * gpu_img.shape[2]
    assert st["pixels_over_1e-4"] <= max(1, int(np.ceil(1e-5 * n))), st
    assert st["all_flagged"], st
    assert st["max_unflagged"] <= 2e-6, st
    print(f"[parity vs libm expf] {gpu_img.shape[2]}x{gpu_img.shape[1]}: {st}")
    return st


def libm_parity_stats(gpu_img, ref):
    with np.errstate(invalid="ignore"):
        diff = np.abs(gpu_img.astype(np.float64) - ref["img"].astype(np.float64)).max(axis=0)
    diff = np.where(np.isnan(gpu_img).any(axis=0) & np.isnan(ref["img"]).any(axis=0), 0.0, diff)
    amb = ref["ambig"].astype(bool)
    over = diff > 1e-4
    return {"pixels_over_1e-4": int(over.sum()), "max_abs_diff": float(diff.max()),
            "all_flagged": bool((~over | amb).all()), "ambiguous_pixels": int(amb.sum()),
            "max_unflagged": float(diff[~amb].max()) if (~amb).any() else 0.0}


def assert_parity_vs_numerics_variants(gpu_img, scene, ocam, **render_kw):
    """The HIP frame against the oracle evaluated under the reference's LIKELY numerics (oracle/numerics.py): FMA contraction
    (a CUDA JIT's default), reciprocal-multiply division, rsqrt forms, libm's expf, right-to-left sums.  Such a frame differs
    from the parity oracle's in a few hundred of two million pixels by up to 3e-3 -- threshold, depth-order and rect flips, and
    ill-conditioned splats.  Asserted, per variant: EVERY pixel of the frame lies within the per-pixel bound the checker
    derives from its own evaluations (the continuous first-order term from the measured per-splat uncertainties + what each
    decision inside its rounding window could move the pixel by); the pixels beyond 1e-4 are at most 5e-4 of the frame; and
    the bound is not vacuous: at most 8 % of the frame may move beyond 1e-4 by it.  Four of the variants take no part in
    measuring the uncertainties (numerics.ENSEMBLE): the independent check.  Returns numerics.report's dict."""
    from oracle import numerics

    rep, cl = numerics.report(scene, ocam, img=gpu_img, **render_kw)
    n = gpu_img.shape[1] * gpu_img.shape[2]
    c = rep["classes"]
    assert c["pixels_that_may_move_over_1e_4"] <= 0.08 * n, c
    for name, v in rep["variants"].items():
        assert v["all_explained"], (name, v)
        assert v["pixels_over_1e-4"] <= max(3, int(np.ceil(5e-4 * n))), (name, v)
    vs = rep["variants"]
    print(f"[parity vs numerics variants] {gpu_img.shape[2]}x{gpu_img.shape[1]}: may move > 1e-4: "
          f"{c['pixels_that_may_move_over_1e_4']} of {n} px (flagged: threshold {c['threshold_pixels']}, depth order "
          f"{c['depth_pixels']}, rect {c['rect_pixels']}); " +
          "; ".join(f"{k}: {v['pixels_over_1e-4']} px > 1e-4, max {v['max_abs_diff']:.1e}, worst diff/bound "
                    f"{v['worst_ratio_diff_to_bound']:.2f}" for k, v in vs.items()))
    return rep


def random_draw(seed):
    """One seeded random frame (tests/test_gpu_random_sweep.py, tests/test_oracle_gradient_rows.py): (rng, scene, W, H, pose,
    fov, bg, scale_modifier) -- sizes, resolutions that are not multiples of 16, fields of view, scale distributions (every
    third draw anisotropic needles and a few giants), poses, backgrounds, scale modifiers."""
    from conftest import make_scene

    rng = np.random.default_rng(1000 + seed)
    P = int(rng.integers(1, 4000))
    W, H = int(rng.integers(17, 420)), int(rng.integers(17, 300))
    scene = make_scene(rng, P, spread=float(rng.uniform(0.2, 1.5)),
                       log_scale=(float(rng.uniform(-5.5, -2.0)), float(rng.uniform(0.2, 1.2))))
    if seed % 3 == 0:  # anisotropic needles and a few giants
        scene["scale"][:, 0] *= 8.0
        scene["scale"][: max(1, P // 50)] *= 25.0
    ang, elev, dist = rng.uniform(0, 2 * np.pi), rng.uniform(-0.6, 0.9), rng.uniform(0.3, 6.0)
    pos = [dist * np.cos(ang) * np.cos(elev), dist * np.sin(ang) * np.cos(elev), 0.5 + dist * np.sin(elev)]
    pose = (pos, [0.0, 0.0, 0.5], [0.0, 0.0, 1.0])
    return rng, scene, W, H, pose, float(rng.uniform(20.0, 110.0)), tuple(rng.uniform(0, 1, 3).tolist()), \
        float(rng.uniform(0.5, 1.5))


GRAD_F32_FACTOR = 3.0   # see check_gradients
GRAD_GIANT_BAR = 5e-3


def check_gradients(g, ref32, ref64, P, radii, tag, report=None, flat_bar=None):
    """The kernels' gradients against the f64 oracle -- the ONLY yardstick (the f32 oracle shares the kernels' exp and
    threshold decisions, so agreement with it alone proves nothing about precision).  Bar per attribute, over ALL rows
    (screen-filling giants included since round 4): BASELINE's 1e-3 relative, or -- on ill-conditioned draws, where f32
    arithmetic itself cannot do better -- GRAD_F32_FACTOR x the error the f32 ORACLE makes against f64 on the same rows.

    Why a multiple of the f32 oracle's error, and why 3.  Measured in round 4 (profiles/r04_gradient_error_survey.txt, 1875
    checks of the 1500-draw soak): 237 checks are ill-conditioned (f32 oracle beyond 3e-4, up to 1.7e-1 on draws that plant
    screen-filling splats next to the camera), and the decomposition on the CPU shows WHERE: mostly in the per-splat
    algebra of the preprocess-backward (conic -> covariance -> Sigma -> scale / quaternion: products of 1e5-sized
    covariances and 1e-6-sized conics that cancel), which no f32 evaluation of these formulas escapes -- so the kernels
    evaluate that algebra in f64 for splats whose footprint exceeds ~64 px (backward.hip::geom_backward) -- and, for a few
    draws, in the f32 sums over pixels, which the kernels share with the f32 oracle (another summation order: a second
    sample of the same rounding noise).  With both in place the ratio kernel / f32 oracle over the 237 checks has median
    0.20, 90th percentile 1.00, 99th 1.09, maximum 2.41; every well-conditioned check is below 3.2e-4.  3 covers the tail of
    the shared part; the soak additionally asserts the DISTRIBUTION (median, 90th percentile).
    Rows of giants (radius > 64 px) are held to max(GRAD_GIANT_BAR, 3 x the f32 oracle on those rows) on their own, so
    that they cannot hide inside a large norm either.
    flat_bar: additionally hold every attribute to this figure outright, whatever the f32 oracle does (BASELINE C4 at size:
    5e-4 -- every attribute lands below 3e-4 there, so the f32-relative slack is not needed and not granted).
    report: a list -> nothing is asserted, the figures are appended (soak's survey mode)."""
    rel = lambda x, y: float(np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-30))
    giant = radii > 64
    for k in g:
        a = g[k].detach().cpu().numpy().astype(np.float64).reshape(P, -1)
        assert np.isfinite(a).all(), (tag, k)
        b32 = ref32[k].astype(np.float64).reshape(P, -1)
        b64 = ref64[k].astype(np.float64).reshape(P, -1)
        e, e32 = rel(a, b64), rel(b32, b64)
        eg = rel(a[giant], b64[giant]) if giant.any() and np.linalg.norm(b64[giant]) > 0 else 0.0
        eg32 = rel(b32[giant], b64[giant]) if giant.any() and np.linalg.norm(b64[giant]) > 0 else 0.0
        if report is not None:
            report.append({"tag": tag, "k": k, "e": e, "e32": e32, "eg": eg, "eg32": eg32, "giants": int(giant.sum())})
            continue
        print(f"[gradients vs f64] {tag} {k}: kernels {e:.2e}, f32 oracle {e32:.2e}; {int(giant.sum())} giants: {eg:.2e} / {eg32:.2e}")
        assert e <= max(1e-3, GRAD_F32_FACTOR * e32), (
            f"{tag} {k}: {e:.2e} vs the f64 oracle (f32 oracle vs f64: {e32:.2e}; giants alone {eg:.2e} / {eg32:.2e})")
        assert flat_bar is None or e <= flat_bar, f"{tag} {k}: {e:.2e} vs the f64 oracle, beyond the flat bar {flat_bar:.0e}"
        assert eg <= max(GRAD_GIANT_BAR, GRAD_F32_FACTOR * eg32), (
            f"{tag} {k}: rows of the {int(giant.sum())} giants {eg:.2e} vs f64 (f32 oracle on them: {eg32:.2e})")


# ---------------------------------------------------------------------------------------------------------------- per row
GRAD_ROW_K = 3.0      # x the f32 oracles' own error on the component (the larger of the two builds')
GRAD_ROW_CU = 128.0   # x u x (|J| A): summation order, the drift of T, the hardware exp's error in every G
GRAD_ROW_FLOOR = 1e-7  # x (|J| A): an absolute floor, not a tolerance
U32 = 2.0 ** -24
_ORACLES = {}


def _oracles():
    if not _ORACLES:
        from oracle import Oracle

        _ORACLES.update(f32=Oracle("f32"), f64=Oracle("f64"), f32c=Oracle("f32", contracted=True))
    return _ORACLES["f32"], _ORACLES["f64"], _ORACLES["f32c"]


def gradient_row_bound(scene, ocam, dL, bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3, ref32=None, ref64=None, ref32c=None,
                       cam64=None):
    """(per attribute [P, n] bound B, ref64) of check_gradient_rows, for one view.  ref32 / ref64 / ref32c: the oracles'
    render_backward_full of the same view when the caller has them (f32, f64, contracted f32); computed otherwise.
    cam64: the f64 oracle's own camera (default: ocam widened)."""
    from oracle import gradient_row_terms

    o32, o64, o32c = _oracles()
    ocam = o32.convert_camera(ocam)
    kw = dict(bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    if ref32 is None:
        ref32 = o32.render_backward_full(scene, ocam, dL, **kw)
    if ref64 is None:
        ref64 = o64.render_backward_full(scene, cam64 if cam64 is not None else o64.convert_camera(ocam), dL, **kw)
    if ref32c is None:
        ref32c = o32c.render_backward_full(scene, o32c.convert_camera(ocam), dL, **kw)
    t = gradient_row_terms(o32, o64, scene, ocam, dL, **kw)
    P = np.asarray(scene["pos"]).reshape(-1, 3).shape[0]
    B = {}
    for k in ("pos", "scale", "rotq", "sh", "opacity"):
        b64 = ref64[k].astype(np.float64).reshape(P, -1)
        noise = np.maximum(np.abs(ref32[k].astype(np.float64).reshape(P, -1) - b64),
                           np.abs(ref32c[k].astype(np.float64).reshape(P, -1) - b64))
        JA, JF = t["JA"][k].reshape(P, -1), t["JF"][k].reshape(P, -1)
        B[k] = GRAD_ROW_K * noise + GRAD_ROW_CU * U32 * JA + JF + GRAD_ROW_FLOOR * JA
    return B, ref64


def gradient_row_ratios(got, B, ref64, rows=None):
    """per attribute: (worst |a - b64| / B, its row, rows over the bound).  got: attribute -> array or tensor; rows: the
    oracle rows that got's rows hold (compact gradients), default all."""
    out = {}
    for k, bound in B.items():
        a = got[k]
        a = (a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)).astype(np.float64)
        b64 = ref64[k].astype(np.float64).reshape(bound.shape[0], -1)
        if rows is not None:
            b64, bound = b64[rows], bound[rows]
        a = a.reshape(b64.shape[0], -1)
        diff = np.abs(a - b64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
        r = np.where(np.isfinite(a), r, np.inf).max(axis=1)
        i = int(np.argmax(r)) if r.size else 0
        bad = np.nonzero(r > 1.0)[0]
        out[k] = (float(r[i]) if r.size else 0.0, int(rows[i]) if rows is not None and r.size else i,
                  (np.asarray(rows)[bad] if rows is not None else bad))
    return out


def check_gradient_rows(g, scene, ocam, dL, bg=(0.0, 0.0, 0.0), scale_modifier=1.0, tag="", sh_deg=3, ref32=None, ref64=None,
                        ref32c=None, rows=None, bound=None, report=None, cam64=None):
    """The kernels' gradients held ROW BY ROW, every component of every row, against the f64 oracle:

        |a_i - b64_i| <= K max(|b32_i - b64_i|, |b32c_i - b64_i|) + c_u u (|J| A)_i + (|J| F)_i + 1e-7 (|J| A)_i

    for every component i of every row.  b32 / b32c: the f32 oracle and its contracted-FMA build (two samples of binary32
    noise, incl. the f32/f64 forward's own decisions -- the kernels' forward is the f32 oracle's bit for bit, so what it
    moves, it moves for them too).  A, F: the render-backward
    walk's rounding budget per 2-D component (oracle/lcgs_oracle_bwd.c, orc_set_backward_bound), F for decisions within
    rounding of a threshold; |J|: the per-row Jacobian of the preprocess-backward (oracle.abs_jacobian_apply).  K, c_u:
    GRAD_ROW_K, GRAD_ROW_CU, chosen once on the CPU (tests/test_oracle_gradient_rows.py).  A norm over all rows lets a
    handful of wrong rows through; this does not.
    g: attribute -> kernel gradients (tensors or arrays); rows: the oracle rows g holds (compact rows); bound: a
    precomputed (B, ref64) of gradient_row_bound (sums of views: add the views' B, and their ref64).
    report: a list -> nothing asserted, the worst ratios appended.  Returns attribute -> (worst ratio, its row)."""
    import time

    t0 = time.perf_counter()
    B, r64 = bound if bound is not None else gradient_row_bound(scene, ocam, dL, bg, scale_modifier, sh_deg, ref32, ref64,
                                                                ref32c, cam64)
    res = gradient_row_ratios(g, B, r64, rows)
    worst = {k: (v[0], v[1]) for k, v in res.items()}
    if report is not None:
        report.append({"tag": tag, **{k: v[0] for k, v in res.items()}})
        return worst
    print(f"[gradient rows vs f64] {tag}: worst diff/bound " + ", ".join(f"{k} {v[0]:.3f} (row {v[1]})" for k, v in res.items()) +
          f"; {time.perf_counter() - t0:.2f} s")
    for k, (w, i, bad) in res.items():
        assert w <= 1.0, f"{tag} {k}: {len(bad)} rows over their bound, worst row {i} at {w:.2f} x (rows {bad[:12].tolist()})"
    return worst


# ------------------------------------------------------------------------------- views shared by the per-row route tests
KEYS = ("pos", "scale", "rotq", "sh", "opacity")
BG = (0.1, 0.2, 0.3)
_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class View:
    """One (scene, pose, resolution, dL/dimg): the oracle's frame and the per-row bound, each computed once and then shared."""

    def __init__(self, oracle, scene, pose, W, H, seed=0, bg=BG, sh_deg=3, dL=None, ref=None):
        self.oracle, self.scene, self.pose, self.W, self.H, self.bg, self.sh_deg = oracle, scene, pose, W, H, bg, sh_deg
        self.P = scene["pos"].shape[0]
        self.ocam = oracle.lookat(*pose, width=W, height=H)
        self.ref = ref if ref is not None else oracle.render(scene, self.ocam, bg=bg, sh_deg=sh_deg)
        # `on`: the rows whose tile rectangle is not empty.  (radii > 0 alone also holds for a row in front of the camera whose
        # rectangle misses the frame, which no list ever holds.)  The kernels' cull additionally drops a row whose rectangle,
        # pruned by its opacity, is empty -- the oracle has no such rule, so the frame's survivors lie between `hit` (rows that
        # reach a pixel: their gradient is not 0) and `on`; where a case needs an exact count it asserts that the two agree.
        m2, depth, cov = oracle.project(scene["pos"], scene["scale"], scene["rotq"], self.ocam)
        self.on = oracle.allocate_tiles(W, H, depth, m2, cov)[2] > 0
        self.V = int(self.on.sum())
        self.dL = dL if dL is not None else np.random.default_rng(seed).normal(size=(3, H, W)).astype(np.float32)
        self._bound = self._ref32 = None

    def other_dL(self, seed):
        return View(self.oracle, self.scene, self.pose, self.W, self.H, seed, self.bg, self.sh_deg, ref=self.ref)

    def cam(self):
        import luisacomputegaussiansplatting_amd as L

        return L.get_lookat_cam(*self.pose, width=self.W, height=self.H)

    def ref32(self):
        if self._ref32 is None:
            self._ref32 = self.oracle.render_backward_full(self.scene, self.ocam, self.dL, bg=self.bg, sh_deg=self.sh_deg)
        return self._ref32

    @property
    def hit(self):
        """rows that reach at least one pixel of the f32 oracle's frame (the kernels' frame, bit for bit)"""
        g = self.ref32()
        return (g["opacity"] != 0) | (g["sh"].reshape(self.P, -1) != 0).any(axis=1)

    def bound(self):
        if self._bound is None:
            self._bound = gradient_row_bound(self.scene, self.ocam, self.dL, bg=self.bg, sh_deg=self.sh_deg, ref32=self.ref32())
        return self._bound

    def survivors(self, r):
        """the frame's on-screen rows (lcgs_visible_rows), between `hit` and `on`"""
        rows = r.visible_rows().cpu().numpy()
        assert r.frame_stats()["num_visible"] == rows.size
        got = np.zeros(self.P, bool)
        got[rows] = True
        assert (rows[1:] > rows[:-1]).all() and not (got & ~self.on).any() and not (self.hit & ~got).any(), \
            (rows.size, self.V, int(self.hit.sum()))
        return rows


def sum_bounds(views):
    """the bound of a sum of views: the sum of the views' bounds, against the sum of their f64 references"""
    bs = [v.bound() for v in views]
    return ({k: sum(b[0][k] for b in bs) for k in KEYS}, {k: sum(b[1][k].astype(np.float64) for b in bs) for k in KEYS})


def sevens(scene, sh_offset=0):
    """gradient arrays the backward must overwrite; sh_offset: dL_dsh starts that many floats past a 16-byte boundary"""
    g = {k: torch.full(scene[k].shape, 7.0, device=DEV) for k in KEYS}
    if sh_offset:
        flat = torch.full((scene["sh"].size + 4,), 7.0, device=DEV)
        g["sh"] = flat[sh_offset:sh_offset + scene["sh"].size].view(scene["sh"].shape)
        assert g["sh"].data_ptr() % 16 == 4 * sh_offset and g["sh"].is_contiguous()
    return g
