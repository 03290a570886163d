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
per row at o.dtype and gc + dgc goes in.  tests/test_antialias_ref.py pins the result against central differences."""
import numpy as np

import camera_grad_ref

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
        D = a * c - b * b + dt(np.float32(1e-6))
        iD2 = one / (D * D)
        # (g00, g11, g01) = M (gA, gB, gC): orc_preprocess_backward's "conic -> filtered cov" lines
        M = np.empty((P, 3, 3), dt)
        M[:, 0, 0], M[:, 0, 1], M[:, 0, 2] = -c * c * iD2, b * c * iD2, (D - a * c) * iD2
        M[:, 1, 0], M[:, 1, 1], M[:, 1, 2] = (D - a * c) * iD2, a * b * iD2, -a * a * iD2
        M[:, 2, 0], M[:, 2, 1], M[:, 2, 2] = two * b * c * iD2, -(D + two * b * b) * iD2, two * a * b * iD2
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
