"""The reference of the depth-distortion map (include/lcgs_hip.h, kernels/maps.hip: lcgs_render_distortion) and of its backward,
composed from the UNCHANGED CPU oracle the way maps_ref.py composes depth and alpha, and the per-row bound the kernels' gradients
are held to.  No GPU needed.

Forward: the oracle's forward state composited once more with the per-splat "colour" (u, 1, u^2), u = v - center, over a zero
background: channel 0 is M1 = sum w u, channel 1 A = sum w, channel 2 M2 = sum w u^2, in the renderer's own order, and
dist = A M2 - M1 M1 -- every operation in o.dtype, so the f32 build is what the kernel must equal bit for bit.
Backward, per oracle build: dist is a function of the three composited channels, so its gradient is render_backward with that
colour and the per-pixel incoming gradient g (d dist/dM1, d dist/dA, d dist/dM2) = (-2 g M1, g M2, g A) from the build's own
maps, the preprocess-backward with a zero colour gradient, and the colour's own dependence on the position,
dL/dpos += (dL/du + 2 u dL/du^2) dv/dz front.  A depth or alpha gradient of the same call is maps_ref.backward's, added: its
colour is v, not u, so it cannot ride in the same composition unless center is 0.
Bound: maps_ref.row_bound's formula and constants.  A and F from the f64 walk over the f32 state with the three-channel colour
and incoming gradient -- which takes every part by absolute value, |g M2| + |g A| u^2 + 2 |g M1| |u|, the un-cancelled
magnitudes the kernel's own expression M2 + u (A u - 2 M1) rounds over; columns 6 and 8 go to the position through |dv/dz| and
2 |u| |dv/dz|, column 7 (the constant channel) is dropped.  The other channels' bounds are added."""
import numpy as np

import maps_ref
from gpu_util import GRAD_ROW_CU, GRAD_ROW_FLOOR, GRAD_ROW_K, KEYS, U32, _oracles, gradient_row_bound

MODES = maps_ref.MODES
sum_row_bounds = maps_ref.sum_row_bounds


def _colour(o, v, center):
    """(u [P], colour [P, 3] = (u, 1, u^2)) in o.dtype: one subtraction and one product per splat; center is a binary32 number"""
    u = (v - o.dtype(np.float32(center))).astype(o.dtype)
    return u, np.stack([u, np.ones_like(u), (u * u).astype(o.dtype)], axis=1)


def compose(o, st, cam, v, center):
    """(dist, A, M1, M2), [H, W] each in o.dtype, of a forward state `st` (Oracle.forward_state's, or antialias_ref's)"""
    img = o.render_forward(cam.width, cam.height, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"],
                           st["opacity"], _colour(o, v, center)[1])[0]
    M1, A, M2 = img[0], img[1], img[2]
    dist = A * M2 - M1 * M1
    assert dist.dtype == o.dtype
    return dist, A, M1, M2


def forward(o, scene, cam, mode="z", center=0.0, scale_modifier=1.0, sh_deg=3):
    """(dist [H, W], forward state) of oracle build `o`"""
    st = o.forward_state(scene, cam, scale_modifier=scale_modifier, sh_deg=sh_deg)
    v, _ = maps_ref._value(o, scene, cam, mode, scale_modifier)
    return compose(o, st, cam, v, center)[0], st


def _walk_inputs(o, st, cam, v, center, dL_ddist):
    """(colour, incoming gradient [3, H, W]) of the distortion channel, from the maps of build `o` over the state `st`"""
    _, A, M1, M2 = compose(o, st, cam, v, center)
    g = np.asarray(dL_ddist, o.dtype)
    two = o.dtype(2.0)
    return _colour(o, v, center)[1], np.stack([-(two * g * M1), g * M2, g * A]).astype(o.dtype)


def backward(o, scene, cam, dL_ddist, dL_ddepth=None, dL_dalpha=None, mode="z", center=0.0, scale_modifier=1.0, sh_deg=3,
             frame=maps_ref.Classic, walk=None):
    """attribute -> gradient of <dL_ddist, dist> + <dL_ddepth, depth> + <dL_dalpha, alpha> in oracle build `o` (its own forward);
    frame: maps_ref.Classic, or another raster mode's state and augmentation; walk: a dict that receives the distortion walk's
    own dL/dopacity row ("go")"""
    W, H = cam.width, cam.height
    st = frame.state(o, scene, cam, scale_modifier, sh_deg)
    v, dv = maps_ref._value(o, scene, cam, mode, scale_modifier)
    u = _colour(o, v, center)[0]
    col, dl3 = _walk_inputs(o, st, cam, v, center, dL_ddist)
    gm, gc, go, gcol = o.render_backward(W, H, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"],
                                         st["opacity"], col, st["final_T"], st["n_contrib"], dl3)
    if walk is not None:
        walk["go"] = go
    gc, go = frame.augment(o, st, gc, go)
    g = o.preprocess_backward(scene, cam, st["radii"], gm, gc, np.zeros_like(gcol), scale_modifier=scale_modifier, sh_deg=sh_deg)
    gu = gcol[:, 0] + o.dtype(2.0) * u * gcol[:, 2]
    g["pos"] = g["pos"] + (gu * dv)[:, None] * np.asarray(cam.front[:], o.dtype)[None, :]
    g["opacity"] = go
    g["sh"] = np.zeros_like(g["sh"])
    if dL_ddepth is not None or dL_dalpha is not None:
        gm_ = maps_ref.backward(o, scene, cam, dL_ddepth, dL_dalpha, mode=mode, scale_modifier=scale_modifier, sh_deg=sh_deg,
                                frame=frame)
        g = {k: g[k] + gm_[k] for k in g}
    return g


def row_bound(scene, ocam, dL_ddist, dL_ddepth=None, dL_dalpha=None, mode="z", center=0.0, scale_modifier=1.0, sh_deg=3,
              maps_bound=None, frame=maps_ref.Classic):
    """(per attribute [P, n] bound, f64 reference) for a distortion backward without an image gradient.  maps_bound: the
    (bound, reference) of maps_ref.row_bound for the same dL_ddepth / dL_dalpha, where the caller has it."""
    from oracle import abs_jacobian_apply

    o32, o64, o32c = _oracles()
    ocam = o32.convert_camera(ocam)
    cam64 = o64.convert_camera(ocam)
    kw = dict(mode=mode, center=center, scale_modifier=scale_modifier, sh_deg=sh_deg, frame=frame)
    r32 = backward(o32, scene, ocam, dL_ddist, **kw)
    walk64 = {}
    r64 = backward(o64, scene, cam64, dL_ddist, walk=walk64, **kw)
    r32c = backward(o32c, scene, o32c.convert_camera(ocam), dL_ddist, **kw)
    # the rounding budget of the walk, over the binary32 state and the binary32 maps the kernels produce bit for bit
    W, H = ocam.width, ocam.height
    st = frame.state(o32, scene, ocam, scale_modifier, sh_deg)
    v, dv = maps_ref._value(o32, scene, ocam, mode, scale_modifier)
    u = _colour(o32, v, center)[0]
    col, dl3 = _walk_inputs(o32, st, ocam, v, center, dL_ddist)
    A, F = o64.render_backward_bound(W, H, np.zeros(3, np.float32), st["ranges"], st["point_list"], st["means"], st["conic"],
                                     st["opacity"], col, st["final_T"], st["n_contrib"], dl3)
    A, F = (frame.augment_budget(o64, scene, cam64, st, X, scale_modifier) for X in (A, F))
    Az, Fz = A.copy(), F.copy()
    Az[:, 6:9] = 0.0
    Fz[:, 6:9] = 0.0
    JA, JF = abs_jacobian_apply(o64, scene, cam64, st["radii"], (Az, Fz), scale_modifier, sh_deg)
    front = np.abs(np.asarray(cam64.front[:], np.float64))[None, :]
    adv = np.abs(dv.astype(np.float64))
    au2 = 2.0 * np.abs(u.astype(np.float64))
    JA["pos"] = JA["pos"] + ((A[:, 6] + au2 * A[:, 8]) * adv)[:, None] * front
    JF["pos"] = JF["pos"] + ((F[:, 6] + au2 * F[:, 8]) * adv)[:, None] * front
    P = np.asarray(scene["pos"]).reshape(-1, 3).shape[0]
    extra = frame.conditioning(o64, scene, cam64, st["radii"], walk64["go"], scale_modifier, sh_deg)
    B, R = {}, {}
    for k in KEYS:
        b64 = r64[k].astype(np.float64).reshape(P, -1)
        noise = np.maximum(np.abs(r32[k].astype(np.float64).reshape(P, -1) - b64),
                           np.abs(r32c[k].astype(np.float64).reshape(P, -1) - b64))
        ja, jf = JA[k].reshape(P, -1), JF[k].reshape(P, -1)
        B[k] = GRAD_ROW_K * noise + GRAD_ROW_CU * U32 * ja + jf + GRAD_ROW_FLOOR * ja
        if extra is not None:
            B[k] = B[k] + extra[k].reshape(P, -1)
        R[k] = b64
    if dL_ddepth is not None or dL_dalpha is not None:
        if maps_bound is None:
            maps_bound = maps_ref.row_bound(scene, ocam, dL_ddepth, dL_dalpha, mode, scale_modifier, sh_deg, frame=frame)
        return sum_row_bounds([(B, R), maps_bound])
    return B, R


def row_bound_with_image(scene, ocam, dL_dimg, dL_ddist, dL_ddepth=None, dL_dalpha=None, mode="z", center=0.0,
                         bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3, maps_bound=None, image_bound=None):
    """a call that also passes dL_dimg: the sum of the bounds, against the sum of the f64 references"""
    Bd = row_bound(scene, ocam, dL_ddist, dL_ddepth, dL_dalpha, mode, center, scale_modifier, sh_deg, maps_bound)
    if image_bound is None:
        image_bound = gradient_row_bound(scene, ocam, dL_dimg, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    return sum_row_bounds([Bd, image_bound])
