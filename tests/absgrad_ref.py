"""The reference of the AbsGS densification statistic (include/lcgs_hip.h lcgs_absgrad_accumulate, kernels/absgrad.hip), composed
from the UNCHANGED CPU oracle the way maps_ref.py and features_ref.py are, and the per-row bound the kernel's sums are held to.
No GPU needed.

Definition: g(p, .) -- the gradient of the part of L = <dL_dimg, img> + <dL_ddepth, depth> + <dL_dalpha, alpha> that belongs to
pixel p with respect to every row's pixel-space mean -- IS what Oracle.render_backward(...)[0] returns for a dL that is zero
outside pixel p.  The colour walk uses the frame's colours and background; the map channels are a second walk with
maps_ref._colour(v) and (dL_ddepth, dL_dalpha, 0) over a zero background.  The two are added per pixel, then abs, then summed
over p:  a_i = (sum_p |g_x(p, i)|, sum_p |g_y(p, i)|).  `sums` also returns the two statistics a wrong kernel would compute --
the signed one, |sum_p g|, and the per-tile one, sum_tiles |sum_{p in tile} g| (the absolute value taken at the flush) -- so that
tests/test_absgrad_ref.py can show that the bound tells them apart.

A one-hot walk is run over a copy of the state whose n_contrib is zero outside p: the oracle then walks one pixel's list instead
of all of them (a pixel whose dL is zero adds exact zeros either way; test_absgrad_ref.py holds the shortcut to the plain one-hot
call bit for bit).  `frame`: maps_ref.Classic or antialias_ref.Antialiased, the state the walks run over.

Bound, per row and component, with the project's constants and formula and no Jacobian (the statistic is a 2-D quantity):
    B = GRAD_ROW_K max(|abs32 - abs64|, |abs32c - abs64|) + GRAD_ROW_CU U32 A + F + GRAD_ROW_FLOOR A
A, F: columns 0:2 of the f64 oracle's render_backward_bound over the f32 state with the full dL, summed over the two walks.  A sums
|term| (1 + depth) per pixel: it bounds the rounding of the absolute sum as it does the signed one."""
import numpy as np

import maps_ref
from gpu_util import GRAD_ROW_CU, GRAD_ROW_FLOOR, GRAD_ROW_K, U32, _oracles
from maps_ref import Classic

TILE = 16


def _walks(o, st, scene, cam, dL_dimg, dL_ddepth, dL_dalpha, mode, bg, scale_modifier):
    """[(background, per-splat colour, dL [3, H, W])] of the walks the call is made of, at o.dtype"""
    W, H = cam.width, cam.height
    walks = []
    if dL_dimg is not None:
        walks.append((np.asarray(bg, o.dtype), st["color"], np.ascontiguousarray(dL_dimg, o.dtype)))
    if dL_ddepth is not None or dL_dalpha is not None:
        v, _ = maps_ref._value(o, scene, cam, mode, scale_modifier)
        walks.append((np.zeros(3, o.dtype), maps_ref._colour(v), maps_ref._dl3(o, dL_ddepth, dL_dalpha, H, W)))
    assert walks, "all three gradients are None"
    return walks


def pixel_gradient(o, st, W, H, walks, x, y, shortcut=True):
    """g(p, .) [P, 2] at o.dtype for p = (x, y): the walks' one-hot render_backward, added"""
    g = None
    nc = st["n_contrib"]
    if shortcut:
        nc = np.zeros_like(st["n_contrib"])
        nc.reshape(H, W)[y, x] = np.asarray(st["n_contrib"]).reshape(H, W)[y, x]
    for bg, colour, dL in walks:
        one = np.zeros_like(dL)
        one[:, y, x] = dL[:, y, x]
        gm = o.render_backward(W, H, bg, st["ranges"], st["point_list"], st["means"], st["conic"], st["opacity"], colour,
                               st["final_T"], nc, one)[0]
        g = gm if g is None else g + gm
    return g


def sums(o, scene, cam, dL_dimg=None, dL_ddepth=None, dL_dalpha=None, mode="z", bg=(0.0, 0.0, 0.0), frame=Classic,
         scale_modifier=1.0, sh_deg=3, shortcut=True):
    """dict(abs, signed, tiles [P, 2] at o.dtype, accumulated at o.dtype; full [P, 2]: the walks' plain render_backward, added;
    state) of oracle build `o` over its own forward"""
    W, H = cam.width, cam.height
    st = frame.state(o, scene, cam, scale_modifier, sh_deg)
    walks = _walks(o, st, scene, cam, dL_dimg, dL_ddepth, dL_dalpha, mode, bg, scale_modifier)
    P = np.asarray(st["means"]).reshape(-1, 2).shape[0]
    a, s, t = (np.zeros((P, 2), o.dtype) for _ in range(3))
    for ty in range(0, H, TILE):
        for tx in range(0, W, TILE):
            tile = np.zeros((P, 2), o.dtype)
            for y in range(ty, min(ty + TILE, H)):
                for x in range(tx, min(tx + TILE, W)):
                    g = pixel_gradient(o, st, W, H, walks, x, y, shortcut)
                    a += np.abs(g)
                    tile += g
            s += tile
            t += np.abs(tile)
    full = sum(o.render_backward(W, H, b, st["ranges"], st["point_list"], st["means"], st["conic"], st["opacity"], c, st["final_T"],
                                 st["n_contrib"], d)[0] for b, c, d in walks)
    return {"abs": a, "signed": np.abs(s), "sum": s, "tiles": t, "full": full, "state": st}


def reference(scene, ocam, dL_dimg=None, dL_ddepth=None, dL_dalpha=None, mode="z", bg=(0.0, 0.0, 0.0), frame=Classic,
              scale_modifier=1.0, sh_deg=3):
    """dict(abs64, abs32, abs32c, signed64, tiles64 [P, 2] float64; A, F [P, 2]; B [P, 2]: the bound on |kernel - abs64|;
    r32, r64: the builds' `sums`) for one call of lcgs_absgrad_accumulate"""
    o32, o64, o32c = _oracles()
    ocam = o32.convert_camera(ocam)
    kw = dict(mode=mode, bg=bg, frame=frame, scale_modifier=scale_modifier, sh_deg=sh_deg)
    r32 = sums(o32, scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, **kw)
    r64 = sums(o64, scene, o64.convert_camera(ocam), dL_dimg, dL_ddepth, dL_dalpha, **kw)
    r32c = sums(o32c, scene, o32c.convert_camera(ocam), dL_dimg, dL_ddepth, dL_dalpha, **kw)
    # the rounding budget of the walks, over the binary32 state the kernels' forward produces bit for bit
    W, H = ocam.width, ocam.height
    st = r32["state"]
    A, F = np.zeros((st["means"].shape[0], 2)), np.zeros((st["means"].shape[0], 2))
    for b, c, d in _walks(o32, st, scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, mode, bg, scale_modifier):
        a, f = o64.render_backward_bound(W, H, np.asarray(b, np.float32), st["ranges"], st["point_list"], st["means"], st["conic"],
                                         st["opacity"], c, st["final_T"], st["n_contrib"], d)
        A += a[:, 0:2]
        F += f[:, 0:2]
    a64 = r64["abs"].astype(np.float64)
    noise = np.maximum(np.abs(r32["abs"].astype(np.float64) - a64), np.abs(r32c["abs"].astype(np.float64) - a64))
    B = GRAD_ROW_K * noise + GRAD_ROW_CU * U32 * A + F + GRAD_ROW_FLOOR * A
    return {"abs64": a64, "abs32": r32["abs"].astype(np.float64), "abs32c": r32c["abs"].astype(np.float64),
            "signed64": r64["signed"].astype(np.float64), "tiles64": r64["tiles"].astype(np.float64), "A": A, "F": F, "B": B,
            "r32": r32, "r64": r64}


def ratios(got, ref, scale=1.0):
    """|got - scale abs64| / (scale B) per row and component [P, 2]; a difference over a zero bound is inf"""
    diff = np.abs(np.asarray(got, np.float64).reshape(-1, 2) - scale * ref["abs64"])
    bound = scale * ref["B"]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, diff / bound, np.where(diff > 0, np.inf, 0.0))
    return np.where(np.isfinite(np.asarray(got, np.float64).reshape(-1, 2)), r, np.inf)


def stats_bound(refs, W, H):
    """(want [P], bound [P]) of grad_accum over the calls `refs`: sum of |(a_x W/2, a_y H/2)|, and (B_x W/2 + B_y H/2) summed
    (|norm a - norm b| <= |a_x - b_x| + |a_y - b_y|), as tests/test_gpu_densify.py does"""
    half = np.array([W / 2, H / 2])
    want = sum(np.sqrt(((r["abs64"] * half) ** 2).sum(axis=1)) for r in refs)
    bound = sum((r["B"] * half).sum(axis=1) for r in refs)
    return want, bound


# ---------------------------------------------------------------------------------------------------------------- the frames
POSE = ([0.0, 0.0, -4.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0])  # at (0, 0, -4), looking at the origin
BG = (0.1, 0.2, 0.3)


def scene300():
    from conftest import make_scene

    return make_scene(np.random.default_rng(5), 300)


def gradients(W, H, seed, colour=True, depth=True, alpha=True):
    """(dL_dimg [3, H, W], dL_ddepth [H, W], dL_dalpha [H, W]) float32 normals, None where not asked for"""
    rng = np.random.default_rng(seed)
    di, dd, da = (rng.normal(size=s).astype(np.float32) for s in ((3, H, W), (H, W), (H, W)))
    return (di if colour else None, dd if depth else None, da if alpha else None)
