"""The reference of the antialiased raster mode (lcgs_set_raster_mode, include/lcgs_hip.h), composed from the UNCHANGED CPU oracle
the way maps_ref.py and camera_grad_ref.py are.  No GPU needed.

The mode keeps the 0.3 px^2 dilation of the projected covariance and blends with o' = opacity * rho,
    d0  = cov[0] cov[2] - cov[1]^2            cov: what o.project returns (the projector's raw covariance)
    d1  = filt[0] filt[2] - filt[1]^2         filt: cov with 0.3 added on the diagonal
    rho = sqrt(max(0, d0 / d1))               a NaN quotient gives 0
in numpy at o.dtype: for the f32 oracle these are the binary32 operations of the kernels (gs_math.hpp aa_compensation), one
rounding each.  Everything else -- radii, tiles, keys, lists -- is the classic frame's.

Gradients: o.render_backward over that state gives (gm, gc, go', gcol) with go' = dL/do'.  Then dL/dopacity = go' rho, and with
a, c filtered, a0 = a - 0.3, c0 = c - 0.3, k = go' opacity / (2 rho d1^2) (rho == 0: nothing), the covariance (a, b, c) receives
    e00 = k (c0 d1 - d0 c)      e11 = k (a0 d1 - d0 a)      e01 = k 2 b (d0 - d1)
on top of what the conic hands it.  o.preprocess_backward takes dL/dconic, not dL/dcov, and conic = (c, -b, a) / D is locally
invertible: the rows of its Jacobian are orc_preprocess_backward's own (g00, g11, g01 of (gA, gB, gC)), so M dgc = e is solved
per row at o.dtype and gc + dgc goes in.  tests/test_antialias_ref.py pins the result against central differences.

Per-row bound (row_bound, maps_row_bound, distortion_row_bound, camera_bound): gpu_util.check_gradient_rows' formula and constants
carried through that linear map, plus one counted term for the determinants the kernels' backward recomputes -- see "the
per-row bound" and "the determinants' rounding budget" below.  The depth, alpha and distortion channels are maps_ref's and
distortion_ref's own functions handed this module's state and augmentation (`Antialiased`)."""
import numpy as np

import camera_grad_ref
import distortion_ref
import maps_ref
from conftest import make_scene
from gpu_util import GRAD_ROW_CU, GRAD_ROW_FLOOR, GRAD_ROW_K, U32, _oracles
from maps_ref import crowd
from oracle import abs_jacobian_apply

KEYS = ("pos", "scale", "rotq", "sh", "opacity")


def compensation(o, cov):
    """dict(rho, d0, d1, a0, b, c0, a, c), [P] each at o.dtype, from the raw covariance rows cov [P, 3] = (xx, xy, yy)"""
    dt = o.dtype
    cv = np.asarray(cov, dt).reshape(-1, 3)
    k = dt(np.float32(0.3))  # (the oracle's constants are binary32 literals, widened)
    a0, b, c0 = cv[:, 0], cv[:, 1], cv[:, 2]
    a, c = a0 + k, c0 + k
    with np.errstate(all="ignore"):
        d0 = a0 * c0 - b * b
        d1 = a * c - b * b
        q = d0 / d1
        rho = np.sqrt(np.where(q > 0, q, dt(0.0)))
    assert rho.dtype == dt and d0.dtype == dt
    return {"rho": rho, "d0": d0, "d1": d1, "a0": a0, "b": b, "c0": c0, "a": a, "c": c}


def forward_state(o, scene, cam, bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3):
    """Oracle.forward_state's sequence of stage calls with opacity * rho handed to o.render_forward: its dict (whose "opacity"
    is the compensated one the walks must see) plus rho, opacity_eff, opacity_raw and the compensation's terms ("aa")"""
    pos = o.arr(scene["pos"], (-1, 3))
    P = pos.shape[0]
    W, H = cam.width, cam.height
    color = o.sh_process(np.array(cam.position[:]), pos, o.arr(scene["sh"], (P, -1)), deg=sh_deg)
    m2, depth, cov = o.project(pos, scene["scale"], scene["rotq"], cam, scale_modifier=scale_modifier)
    means, conic, tiles, radii = o.allocate_tiles(W, H, depth, m2, cov)
    offsets = o.inclusive_sum(tiles)
    keys, vals = o.copy_with_keys(W, H, means, offsets, radii, depth)
    keys, vals = o.sort_pairs(keys, vals)
    ranges = o.get_ranges(keys, ((W + 15) // 16) * ((H + 15) // 16))
    aa = compensation(o, cov)
    opacity = o.arr(scene["opacity"], (P,))
    eff = (opacity * aa["rho"]).astype(o.dtype)  # one multiply
    img, final_T, n_contrib, _ = o.render_forward(W, H, bg, ranges, vals, means, conic, eff, color)
    return {"img": img, "radii": radii, "color": color, "means": means, "conic": conic, "opacity": eff, "ranges": ranges,
            "point_list": vals, "final_T": final_T, "n_contrib": n_contrib, "rho": aa["rho"], "opacity_eff": eff,
            "opacity_raw": opacity, "aa": aa, "num_rendered": int(offsets[-1]) if P else 0}


def _conic_to_cov(dt, a, b, c):
    """M [P, 3, 3], (g00, g11, g01) = M (gA, gB, gC): orc_preprocess_backward's "conic -> filtered cov" lines"""
    one, two = dt(1.0), dt(2.0)
    D = a * c - b * b + dt(np.float32(1e-6))
    iD2 = one / (D * D)
    M = np.empty((a.shape[0], 3, 3), dt)
    M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = -c * c * iD2, b * c * iD2, (D - a * c) * iD2
    M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = (D - a * c) * iD2, a * b * iD2, -a * a * iD2
    M[:, 2, 0], M[:, 2, 1], M[:, 2, 2] = two * b * c * iD2, -(D + two * b * b) * iD2, two * a * b * iD2
    return M


def conic_addition(o, aa, go, opacity):
    """dgc [P, 3]: the addition to dL/dconic that hands the covariance the compensation's (e00, e11, e01); rows whose rho is 0
    (or whose system is not finite) get none"""
    dt = o.dtype
    a, b, c, a0, c0, d0, d1, rho = (aa[k] for k in ("a", "b", "c", "a0", "c0", "d0", "d1", "rho"))
    one, two = dt(1.0), dt(2.0)
    P = rho.shape[0]
    with np.errstate(all="ignore"):
        k = np.asarray(go, dt) * np.asarray(opacity, dt) / (two * rho * (d1 * d1))
        e = np.stack([k * (c0 * d1 - d0 * c), k * (a0 * d1 - d0 * a), k * (two * b * (d0 - d1))], axis=1)
        M = _conic_to_cov(dt, a, b, c)
        det = np.linalg.det(M.astype(np.float64))
    ok = (rho > 0) & np.isfinite(e).all(axis=1) & np.isfinite(M).all(axis=(1, 2)) & np.isfinite(det) & (det != 0)
    dgc = np.zeros((P, 3), dt)
    if ok.any():
        dgc[ok] = np.linalg.solve(M[ok], e[ok][:, :, None])[:, :, 0]
    assert dgc.dtype == dt
    return dgc


def gradients(o, scene, cam, dL_dimg, bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3):
    """(g, state, rows): g = dict(pos, scale, rotq, sh, opacity) of <dL_dimg, antialiased frame> in oracle build `o`; rows
    [P, 10] = the augmented 2-D rows in camera_grad_ref's layout (conic columns with the addition, opacity column dL/do')"""
    dt = o.dtype
    W, H = cam.width, cam.height
    st = forward_state(o, scene, cam, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    gm, gc, go, gcol = o.render_backward(W, H, bg, st["ranges"], st["point_list"], st["means"], st["conic"], st["opacity_eff"],
                                         st["color"], st["final_T"], st["n_contrib"], np.asarray(dL_dimg, dt))
    gc_aug = (gc + conic_addition(o, st["aa"], go, st["opacity_raw"])).astype(dt)
    g = o.preprocess_backward(scene, cam, st["radii"], gm, gc_aug, gcol, scale_modifier=scale_modifier, sh_deg=sh_deg)
    g["opacity"] = (go * st["rho"]).astype(dt)
    rows = np.zeros((go.shape[0], camera_grad_ref.N2D), dt)
    rows[:, 0:2], rows[:, 2:5], rows[:, 5], rows[:, 6:9] = gm, gc_aug, go, gcol
    return g, st, rows


def camera_reference(o, scene, cam, dL_dimg, bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3):
    """(the twelve column sums in float64, the per-row terms [P, 12], g): camera_grad_ref.contributions fed the augmented rows,
    its position columns replaced by minus the reference's own dL/dpos rows (as camera_grad_ref.reference does)"""
    g, st, rows = gradients(o, scene, cam, dL_dimg, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    Cm = camera_grad_ref.contributions(o, scene, cam, st["radii"], rows, "z", scale_modifier, sh_deg)
    Cm[:, 0:3] = -g["pos"]
    return Cm.astype(np.float64).sum(axis=0), Cm, g


# ---------------------------------------------------------------------------------------------------------------- the scenes
def subpixel_crowd():
    """maps_ref.crowd()'s cloud and pose with splats a fraction of a pixel wide: nearly every on-screen row has rho < 0.5, a
    third of them rho < 0.1.  (scene, pose, W, H)"""

    _, pose, W, H = crowd()
    return make_scene(np.random.default_rng(5), 1500, spread=0.25, log_scale=(-4.6, 0.5)), pose, W, H


def needle_crowd():
    """the same cloud as needles: one axis 30 times the others, so that d0 = a0 c0 - b^2 cancels (|a0 c0| + b^2 over 1e3 |d0|
    on a hundred rows)"""

    _, pose, W, H = crowd()
    scene = make_scene(np.random.default_rng(5), 1500, spread=0.25, log_scale=(-5.0, 0.5))
    scene["scale"][:, 0] *= 30
    return scene, pose, W, H


RANK1_ROWS = np.arange(17, 1500, 37)[:40]


def rank1_crowd():
    """the sub-pixel crowd with 40 rows, spread over the index range, flattened to a line: scale = (s, 0, 0), a rank-1
    covariance whose d0 is 0 up to rounding"""
    scene, pose, W, H = subpixel_crowd()
    scene["scale"][RANK1_ROWS, 1:] = 0.0
    return scene, pose, W, H


def cancellation(aa):
    """(|a0 c0| + b^2) / |d0| per row: the conditioning of d0, which the kernels' backward recomputes"""
    a0, b, c0, d0 = (aa[k].astype(np.float64) for k in ("a0", "b", "c0", "d0"))
    with np.errstate(all="ignore"):
        return (np.abs(a0 * c0) + b * b) / np.abs(d0)


def maps_forward(o, scene, cam, mode="z", scale_modifier=1.0, sh_deg=3):
    """(depth, alpha, state): maps_ref.forward over the antialiased state"""
    st = forward_state(o, scene, cam, scale_modifier=scale_modifier, sh_deg=sh_deg)
    v, _ = maps_ref._value(o, scene, cam, mode, scale_modifier)
    img = o.render_forward(cam.width, cam.height, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"],
                           st["opacity_eff"], maps_ref._colour(v))[0]
    return img[0], img[1], st


# ------------------------------------------------------------------------------------------------------------ the per-row bound
# gpu_util.check_gradient_rows' bound, K noise + c_u u |J| A + |J| F + 1e-7 |J| A with gpu_util's constants, extended to the
# mode with no new constant.  noise: the three oracle builds' `gradients`.  A, F: the f64 walk's budgets over the f32
# antialiased state (the kernels' forward, bit for bit).  The mode puts one linear map between the walk's rows and the
# preprocess-backward: conic += c_unit dL/do' (conic_addition is linear in dL/do', c_unit its value at dL/do' = 1) and
# dL/dopacity = rho dL/do'.  Its absolute Jacobian carries the budgets: conic columns X[2:5] + |c_unit| X[5], opacity rho64 X[5].
def _f64_terms(o64, scene, cam64, scale_modifier):
    """(rho64 [P], |c_unit| [P, 3]) of the f64 build: the absolute Jacobian of the mode's map from dL/do' to (dL/dopacity, conic)"""
    _, _, cov = o64.project(scene["pos"], scene["scale"], scene["rotq"], cam64, scale_modifier=scale_modifier)
    aa64 = compensation(o64, cov)
    opacity = o64.arr(scene["opacity"], (cov.shape[0],))
    return aa64["rho"], np.abs(conic_addition(o64, aa64, np.ones_like(opacity), opacity))


class Antialiased:
    """maps_ref.Classic's counterpart: the antialiased state, the augmentation, and the budgets through its absolute Jacobian"""

    @staticmethod
    def state(o, scene, cam, scale_modifier, sh_deg):
        return forward_state(o, scene, cam, scale_modifier=scale_modifier, sh_deg=sh_deg)

    @staticmethod
    def augment(o, st, gc, go):
        return (gc + conic_addition(o, st["aa"], go, st["opacity_raw"])).astype(o.dtype), (go * st["rho"]).astype(o.dtype)

    @staticmethod
    def augment_budget(o64, scene, cam64, st, X, scale_modifier):
        rho64, cu = _f64_terms(o64, scene, cam64, scale_modifier)
        Y = np.array(X, np.float64, copy=True)
        Y[:, 2:5] = X[:, 2:5] + cu * X[:, 5:6]
        Y[:, 5] = rho64 * X[:, 5]
        return Y


    @staticmethod
    def conditioning(o64, scene, cam64, radii, go64, scale_modifier, sh_deg):
        return conditioning_bound(o64, scene, cam64, radii, go64, scale_modifier, sh_deg)


# The determinants' rounding budget E: the one term the mode adds to the bound, counted a priori, not fitted.
#
# The kernels' backward does not read the forward's rho: geom_backward_t (kernels/splat_backward.hpp) recomputes the raw
# covariance (a0, b, c0) = T Sigma T^t, then d0 = a0 c0 - b^2, d1 = a c - b^2, rho and the covariance term from them, in another
# operation order than the forward's ewa_cov2d.  d0 is a difference of two products that agree in their leading digits for a
# needle (|a0 c0| + b^2 over 1e3 |d0| on a hundred rows of the needle crowd), so the relative rounding error of a0, b, c0 arrives
# in d0 multiplied by (|a0 c0| + b^2) / |d0|, and the term k = dL/do' opacity / (2 rho d1^2) has rho = sqrt(d0 / d1) in its
# denominator.  The noise term samples this with two binary32 evaluations whose errors are of one rounding's size on such a
# row, which undercounts: on row 1444 of the needle crowd the f64 preprocess-backward fed the binary32 state's d0 (5.2e-5 from
# the f64 build's, 1.5 u times the row's 600) is 2.6e-6 from the f64 reference in dL/dscale[0], the two f32 references 1e-7.
#
# Which roundings the cancellation multiplies.  Up to M = R S and T0, T1 every rounding is a backward error: the kernel
# evaluates exactly a Gaussian with slightly other axes, scales and Jacobian rows, P' = T' M' (2 x 3), and for any such P'
# d0 = det(P' P'^t) is the sum of the squares of its 2 x 2 minors, which moves by its own relative size -- what the two binary32
# references sample as well as they sample anything.  From Sig on the roundings are not of that form: a rounded Sig is no
# longer M M^t, and an entrywise u |Sig| reaches d0 through c0 da0 + a0 dc0 - 2 b db with nothing to cancel it.  Those roundings,
# in geom_backward_t's own operations, each a relative u = 2^-24 of the entry to first order:
#     Sig[r][k] = M M + M M + M M        one product, two additions     3
#     ST0[r] = Sig T0 + Sig T0 + Sig T0  one product, two additions     3
#     a0 = T0 ST0 + T0 ST0 + T0 ST0      one product, two additions     3      N_COV = 9
# b and c0 run through the same operations.  Each product of d0 then carries twice N_COV and its own rounding:
#     |delta d0| <= (2 N_COV + 1) u (|a0 c0| + b^2),    |delta d1| <= (2 N_COV + 1) u (|a c| + b^2)
# (the sums inside a0, b, c0 taken as they are in a quadratic form of a positive semi-definite Sig, without cancellation of
# their own; the final subtraction's rounding, u |d0|, is below the count's last unit).  With ks = dL/do' opacity / (2 rho d1^2)
# and e = (e00, e11, e01) the covariance term, d0 and d1 taken as independent roundings,
#     de00/dd0 = -e00 / (2 d0) - ks c        de00/dd1 = -3 e00 / (2 d1) + ks c0
#     de11/dd0 = -e11 / (2 d0) - ks a        de11/dd1 = -3 e11 / (2 d1) + ks a0
#     de01/dd0 = -e01 / (2 d0) + 2 ks b      de01/dd1 = -3 e01 / (2 d1) - 2 ks b
# so E_cov = |de/dd0| |delta d0| + |de/dd1| |delta d1| in the filtered covariance's gradient (g00, g11, g01), which reaches
# the attributes through |J_conic M^-1| -- the product formed before the absolute value, since the kernels add e to g00 / g11 /
# g01 directly and never round the detour through the conic -- and
#     E_opacity = |dL/do'| rho (|delta d0| / |d0| + |delta d1| / d1) / 2.
# A row with rho = 0 in the f64 build has no term and no E.  E is 0 where nothing cancels to speak of: at (|a0 c0| + b^2) / |d0|
# of 2 it is 19 u x 2 = 2.3e-6 of the covariance term, below the 128 u = 7.6e-6 of |J| A that every row has.
N_COV = 9
N_DET = 2 * N_COV + 1


def conditioning_terms(o64, scene, cam64, go64, scale_modifier):
    """(E_cov [P, 3] in (g00, g11, g01), E_opacity [P], M^-1 [P, 3, 3] conic <- filtered cov), float64; go64 = dL/do' [P]"""
    _, _, cov = o64.project(scene["pos"], scene["scale"], scene["rotq"], cam64, scale_modifier=scale_modifier)
    aa = compensation(o64, cov)
    a, b, c, a0, c0, d0, d1, rho = (aa[k] for k in ("a", "b", "c", "a0", "c0", "d0", "d1", "rho"))
    P = rho.shape[0]
    go = np.asarray(go64, np.float64).reshape(P)
    opacity = o64.arr(scene["opacity"], (P,))
    E, Eo, Minv = np.zeros((P, 3)), np.zeros(P), np.zeros((P, 3, 3))
    with np.errstate(all="ignore"):
        dd0 = N_DET * U32 * (np.abs(a0 * c0) + b * b)
        dd1 = N_DET * U32 * (np.abs(a * c) + b * b)
        ks = go * opacity / (2.0 * rho * (d1 * d1))
        e = np.stack([ks * (c0 * d1 - d0 * c), ks * (a0 * d1 - d0 * a), ks * (2.0 * b * (d0 - d1))], axis=1)
        de0 = np.stack([-e[:, 0] / (2.0 * d0) - ks * c, -e[:, 1] / (2.0 * d0) - ks * a, -e[:, 2] / (2.0 * d0) + 2.0 * ks * b], axis=1)
        de1 = np.stack([-1.5 * e[:, 0] / d1 + ks * c0, -1.5 * e[:, 1] / d1 + ks * a0, -1.5 * e[:, 2] / d1 - 2.0 * ks * b], axis=1)
        Ecov = np.abs(de0) * dd0[:, None] + np.abs(de1) * dd1[:, None]
        Eop = np.abs(go) * rho * 0.5 * (dd0 / np.abs(d0) + dd1 / d1)
        M = _conic_to_cov(np.float64, a, b, c)
        det = np.linalg.det(M)
    ok = (rho > 0) & np.isfinite(Ecov).all(axis=1) & np.isfinite(Eop) & np.isfinite(M).all(axis=(1, 2)) & np.isfinite(det) & (det != 0)
    E[ok], Eo[ok], Minv[ok] = Ecov[ok], Eop[ok], np.linalg.inv(M[ok])
    return E, Eo, Minv


def conditioning_bound(o64, scene, cam64, radii, go64, scale_modifier=1.0, sh_deg=3):
    """attribute -> [P, n]: E (above) through |J_conic M^-1|, J_conic the preprocess-backward's three conic columns
    (oracle.abs_jacobian_apply's unit runs)"""
    E, Eo, Minv = conditioning_terms(o64, scene, cam64, go64, scale_modifier)
    P = E.shape[0]
    cols = []
    for k in range(3):
        unit = np.zeros((P, 3))
        unit[:, k] = 1.0
        cols.append(o64.preprocess_backward(scene, cam64, radii, np.zeros((P, 2)), unit, np.zeros((P, 3)),
                                            scale_modifier=scale_modifier, sh_deg=sh_deg))
    out = {"opacity": Eo.reshape(P, 1), "sh": np.zeros((P, np.asarray(scene["sh"]).reshape(P, -1).shape[1]))}
    for name in ("pos", "scale", "rotq"):
        Jc = np.stack([c[name].astype(np.float64) for c in cols], axis=2)  # [P, n, 3]
        out[name] = np.einsum("pnj,pj->pn", np.abs(np.einsum("pnk,pkj->pnj", Jc, Minv)), E)
    return out


def _bound_from(noise_refs, r64, JA, JF, P, extra=None):
    B, R = {}, {}
    for k in KEYS:
        b64 = r64[k].astype(np.float64).reshape(P, -1)
        noise = np.maximum.reduce([np.abs(r[k].astype(np.float64).reshape(P, -1) - b64) for r in noise_refs])
        ja, jf = JA[k].reshape(P, -1), JF[k].reshape(P, -1)
        B[k] = GRAD_ROW_K * noise + GRAD_ROW_CU * U32 * ja + jf + GRAD_ROW_FLOOR * ja
        if extra is not None:
            B[k] = B[k] + extra[k].reshape(P, -1)
        R[k] = b64
    return B, R


def row_bound(scene, ocam, dL_dimg, bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3, cam64=None):
    """(B, ref64) in gpu_util.gradient_row_bound's layout for the antialiased frame's image gradient"""
    o32, o64, o32c = _oracles()
    ocam = o32.convert_camera(ocam)
    cam64 = cam64 if cam64 is not None else o64.convert_camera(ocam)
    kw = dict(bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    r32, st, _ = gradients(o32, scene, ocam, dL_dimg, **kw)
    r64, _, rows64 = gradients(o64, scene, cam64, dL_dimg, **kw)
    r32c = gradients(o32c, scene, o32c.convert_camera(ocam), dL_dimg, **kw)[0]
    A, F = o64.render_backward_bound(ocam.width, ocam.height, np.asarray(bg, np.float32), st["ranges"], st["point_list"],
                                     st["means"], st["conic"], st["opacity_eff"], st["color"], st["final_T"], st["n_contrib"],
                                     np.asarray(dL_dimg, np.float32))
    A, F = (Antialiased.augment_budget(o64, scene, cam64, st, X, scale_modifier) for X in (A, F))
    JA, JF = abs_jacobian_apply(o64, scene, cam64, st["radii"], (A, F), scale_modifier, sh_deg)
    extra = conditioning_bound(o64, scene, cam64, st["radii"], rows64[:, 5], scale_modifier, sh_deg)
    return _bound_from((r32, r32c), r64, JA, JF, st["rho"].shape[0], extra)


def maps_backward(o, scene, cam, dL_ddepth, dL_dalpha, mode="z", scale_modifier=1.0, sh_deg=3):
    return maps_ref.backward(o, scene, cam, dL_ddepth, dL_dalpha, mode, scale_modifier, sh_deg, frame=Antialiased)


def maps_row_bound(scene, ocam, dL_ddepth, dL_dalpha, mode="z", scale_modifier=1.0, sh_deg=3):
    return maps_ref.row_bound(scene, ocam, dL_ddepth, dL_dalpha, mode, scale_modifier, sh_deg, frame=Antialiased)


def distortion_backward(o, scene, cam, dL_ddist, dL_ddepth=None, dL_dalpha=None, mode="z", center=0.0, scale_modifier=1.0,
                        sh_deg=3):
    return distortion_ref.backward(o, scene, cam, dL_ddist, dL_ddepth, dL_dalpha, mode, center, scale_modifier, sh_deg,
                                   frame=Antialiased)


def distortion_row_bound(scene, ocam, dL_ddist, dL_ddepth=None, dL_dalpha=None, mode="z", center=0.0, scale_modifier=1.0,
                         sh_deg=3, maps_bound=None):
    return distortion_ref.row_bound(scene, ocam, dL_ddist, dL_ddepth, dL_dalpha, mode, center, scale_modifier, sh_deg,
                                    maps_bound=maps_bound, frame=Antialiased)


def sum_row_bounds(bounds):
    """the bound of a sum of calls -- an image gradient beside map channels (maps_ref's and distortion_ref's *_with_image),
    several views: the sum of their bounds, against the sum of their f64 references"""
    P = bounds[0][0]["pos"].shape[0]
    return ({k: sum(b[0][k] for b in bounds) for k in KEYS},
            {k: sum(np.asarray(b[1][k], np.float64).reshape(P, -1) for b in bounds) for k in KEYS})


# --------------------------------------------------------------------------------------------------------------- camera bound
def camera_rows(o, scene, cam, dL_dimg, dL_ddepth, dL_dalpha, mode="z", bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3):
    """(augmented 2-D rows [P, 10], state, dL/dpos [P, 3]) of build `o` over its own antialiased state: camera_grad_ref.walk_rows
    with the mode's augmentation applied once to the summed rows (it is linear in dL/do')"""
    W, H = cam.width, cam.height
    st = forward_state(o, scene, cam, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    P = st["rho"].shape[0]
    g = np.zeros((P, camera_grad_ref.N2D), o.dtype)
    dpos = np.zeros((P, 3), o.dtype)
    if dL_dimg is not None:
        gi, _, rows = gradients(o, scene, cam, dL_dimg, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
        g += rows
        dpos = dpos + gi["pos"]
    if dL_ddepth is not None or dL_dalpha is not None:
        v, _ = maps_ref._value(o, scene, cam, mode, scale_modifier)
        gm, gc, go, gcol = o.render_backward(W, H, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"],
                                             st["opacity_eff"], maps_ref._colour(v), st["final_T"], st["n_contrib"],
                                             maps_ref._dl3(o, dL_ddepth, dL_dalpha, H, W))
        g[:, 0:2] += gm
        g[:, 2:5] += Antialiased.augment(o, st, gc, go)[0]
        g[:, 5] += go
        g[:, 9] += gcol[:, 0]
        dpos = dpos + maps_backward(o, scene, cam, dL_ddepth, dL_dalpha, mode, scale_modifier, sh_deg)["pos"]
    return g, st, dpos


def walk_budgets(st32, scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, mode="z", bg=(0.0, 0.0, 0.0), scale_modifier=1.0):
    """(A, F) [P, 10] of the f64 walks over the f32 antialiased state st32, before the augmentation: camera_grad_ref.walk_budgets'
    sums (the map walk's column 6, dL/dv, sent to the value slot)"""
    o32, o64, _ = _oracles()
    W, H = ocam.width, ocam.height
    P = st32["rho"].shape[0]
    A, F = np.zeros((P, camera_grad_ref.N2D)), np.zeros((P, camera_grad_ref.N2D))
    walk = lambda bg_, col, dl: o64.render_backward_bound(W, H, bg_, st32["ranges"], st32["point_list"], st32["means"],
                                                          st32["conic"], st32["opacity_eff"], col, st32["final_T"],
                                                          st32["n_contrib"], dl)
    if dL_dimg is not None:
        a, f = walk(np.asarray(bg, np.float32), st32["color"], np.asarray(dL_dimg, np.float32))
        A[:, :9] += a
        F[:, :9] += f
    if dL_ddepth is not None or dL_dalpha is not None:
        v, _ = maps_ref._value(o32, scene, ocam, mode, scale_modifier)
        a, f = walk(np.zeros(3, np.float32), maps_ref._colour(v), maps_ref._dl3(o32, dL_ddepth, dL_dalpha, H, W))
        A[:, :6] += a[:, :6]
        F[:, :6] += f[:, :6]
        A[:, 9] += a[:, 6]
        F[:, 9] += f[:, 6]
    return A, F


def camera_bound(scene, ocam, dL_dimg, dL_ddepth=None, dL_dalpha=None, mode="z", bg=(0.0, 0.0, 0.0), scale_modifier=1.0,
                 sh_deg=3, pos_bound=None):
    """(bound [12], r64 [12]): camera_grad_ref.bound's formula and constants fed the augmented rows.  pos_bound: the per-row
    position bound [P, 3] of the same call (row_bound, maps_row_bound or their sum) when the caller has it."""
    o32, o64, o32c = _oracles()
    ocam = o32.convert_camera(ocam)
    cam64 = o64.convert_camera(ocam)
    kw = dict(mode=mode, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    C = []
    for o, cam in ((o64, cam64), (o32, ocam), (o32c, o32c.convert_camera(ocam))):
        g, st, dpos = camera_rows(o, scene, cam, dL_dimg, dL_ddepth, dL_dalpha, **kw)
        c = camera_grad_ref.contributions(o, scene, cam, st["radii"], g, mode, scale_modifier, sh_deg)
        c[:, 0:3] = -dpos
        C.append(c.astype(np.float64))
        if o is o32:
            st32 = st
        if o is o64:
            go64 = g[:, 5]
    c64, c32, c32c = C
    r64 = c64.sum(axis=0)
    noise = np.maximum(np.abs(c32 - c64), np.abs(c32c - c64)).sum(axis=0)
    A, F = walk_budgets(st32, scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, mode, bg, scale_modifier)
    A, F = (Antialiased.augment_budget(o64, scene, cam64, st32, X, scale_modifier) for X in (A, F))
    Js = camera_grad_ref.unit_jacobian(o64, scene, cam64, st32["radii"], mode, scale_modifier, sh_deg)
    J = np.abs(Js)
    JA, JF = np.einsum("pks,ps->k", J, A), np.einsum("pks,ps->k", J, F)
    B = GRAD_ROW_K * noise + GRAD_ROW_CU * U32 * JA + JF + GRAD_ROW_FLOOR * JA
    E, _, Minv = conditioning_terms(o64, scene, cam64, go64, scale_modifier)  # (the determinants' budget, as conditioning_bound)
    B = B + np.einsum("pkj,pj->k", np.abs(np.einsum("pks,psj->pkj", Js[:, :, 2:5], Minv)), E)
    if pos_bound is None:
        parts = []
        if dL_dimg is not None:
            parts.append(row_bound(scene, ocam, dL_dimg, bg, scale_modifier, sh_deg)[0]["pos"])
        if dL_ddepth is not None or dL_dalpha is not None:
            parts.append(maps_row_bound(scene, ocam, dL_ddepth, dL_dalpha, mode, scale_modifier, sh_deg)[0]["pos"])
        pos_bound = sum(parts)
    B[0:3] = np.asarray(pos_bound, np.float64).sum(axis=0)
    return B + U32 * np.abs(r64), r64
