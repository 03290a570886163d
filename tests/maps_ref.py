"""The reference of the depth / alpha maps (include/lcgs_hip.h, kernels/maps.hip) and of their backward, composed from the
UNCHANGED CPU oracle, and the per-row bound the kernels' gradients are held to.  No GPU needed.

Forward: the f32 oracle's forward state composited once more with the per-splat "colour" (v, 1, 0) over a zero background --
channel 0 is the accumulated depth, channel 1 the accumulated opacity, in the renderer's own binary32 order.
Backward, per oracle build (f32, f64, contracted f32): render_backward with that colour and dL = (dL/dD, dL/dA, 0), the
preprocess-backward with a zero colour gradient, and view z = front . pos + tz: dL/dpos += dL/dv dv/dz front.
Bound: gpu_util.check_gradient_rows' formula with the same constants; A and F from the f64 walk over the f32 state with the
same colour and dL, the colour columns kept out of the Jacobian and column 6 (dL/dv) sent to the position instead.
backward and row_bound take an optional `frame`: the state the walks run over and what the walk's conic and opacity rows become
before the preprocess-backward.  The default, Classic, is the classic frame and adds nothing; tests/antialias_ref.py passes the
antialiased mode's."""
import numpy as np

from gpu_util import GRAD_ROW_CU, GRAD_ROW_FLOOR, GRAD_ROW_K, KEYS, U32, _oracles, gradient_row_bound

MODES = ("z", "inv_z")


def _value(o, scene, cam, mode, scale_modifier):
    """per splat: (v, dv/dz) in the oracle's precision; rows at z = 0 (never on a list) get 0 for both"""
    z = o.project(scene["pos"], scene["scale"], scene["rotq"], cam, scale_modifier=scale_modifier)[1]
    if mode == "z":
        return z, np.ones_like(z)
    assert mode == "inv_z", mode
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(z != 0, o.dtype(1.0) / z, o.dtype(0.0)).astype(o.dtype)  # one IEEE division per splat
        dv = np.where(z != 0, -1.0 / (z.astype(np.float64) ** 2), 0.0).astype(o.dtype)
    return v, dv


def _colour(v):
    return np.stack([v, np.ones_like(v), np.zeros_like(v)], axis=1)


def _dl3(o, dL_ddepth, dL_dalpha, H, W):
    z = np.zeros((H, W), o.dtype)
    return np.stack([z if dL_ddepth is None else np.asarray(dL_ddepth, o.dtype),
                     z if dL_dalpha is None else np.asarray(dL_dalpha, o.dtype), z])


class Classic:
    """The frame the walks run over and what its 2-D rows become before the preprocess-backward: the classic frame's, where
    nothing is added.  Another raster mode passes its own (tests/antialias_ref.py: Antialiased) as `frame=`."""

    @staticmethod
    def state(o, scene, cam, scale_modifier, sh_deg):
        return o.forward_state(scene, cam, scale_modifier=scale_modifier, sh_deg=sh_deg)

    @staticmethod
    def augment(o, st, gc, go):
        """(dL/dconic, dL/dopacity) of build `o` from the walk's conic and opacity rows over the state `st`"""
        return gc, go

    @staticmethod
    def augment_budget(o64, scene, cam64, st, X, scale_modifier):
        """a walk budget X [P, >= 6] (A or F) taken through the absolute Jacobian of `augment`"""
        return X

    @staticmethod
    def conditioning(o64, scene, cam64, radii, go64, scale_modifier, sh_deg):
        """attribute -> [P, n] added to the bound for what `augment` recomputes, from the f64 walk's dL/dopacity; None: nothing"""
        return None


def forward(o, scene, cam, mode="z", scale_modifier=1.0, sh_deg=3):
    """(depth [H, W], alpha [H, W], forward state) of oracle build `o` (the f32 build: what the kernels must equal bit for bit)"""
    st = o.forward_state(scene, cam, scale_modifier=scale_modifier, sh_deg=sh_deg)
    v, _ = _value(o, scene, cam, mode, scale_modifier)
    img = o.render_forward(cam.width, cam.height, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"],
                           st["opacity"], _colour(v))[0]
    return img[0], img[1], st


def backward(o, scene, cam, dL_ddepth, dL_dalpha, mode="z", scale_modifier=1.0, sh_deg=3, frame=Classic, walk=None):
    """attribute -> gradient of <dL_ddepth, depth> + <dL_dalpha, alpha> in oracle build `o` (its own forward); walk: a dict
    that receives the walk's own dL/dopacity row ("go"), before `frame` augments it"""
    W, H = cam.width, cam.height
    st = frame.state(o, scene, cam, scale_modifier, sh_deg)
    v, dv = _value(o, scene, cam, mode, scale_modifier)
    gm, gc, go, gcol = o.render_backward(W, H, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"],
                                         st["opacity"], _colour(v), st["final_T"], st["n_contrib"],
                                         _dl3(o, dL_ddepth, dL_dalpha, H, W))
    if walk is not None:
        walk["go"] = go
    gc, go = frame.augment(o, st, gc, go)
    g = o.preprocess_backward(scene, cam, st["radii"], gm, gc, np.zeros_like(gcol), scale_modifier=scale_modifier, sh_deg=sh_deg)
    g["pos"] = g["pos"] + (gcol[:, 0] * dv)[:, None] * np.asarray(cam.front[:], o.dtype)[None, :]
    g["opacity"] = go
    g["sh"] = np.zeros_like(g["sh"])
    return g


def row_bound(scene, ocam, dL_ddepth, dL_dalpha, mode="z", scale_modifier=1.0, sh_deg=3, frame=Classic):
    """(per attribute [P, n] bound, f64 reference) for a maps backward without an image gradient"""
    from oracle import abs_jacobian_apply

    o32, o64, o32c = _oracles()
    ocam = o32.convert_camera(ocam)
    cam64 = o64.convert_camera(ocam)
    kw = dict(mode=mode, scale_modifier=scale_modifier, sh_deg=sh_deg, frame=frame)
    r32 = backward(o32, scene, ocam, dL_ddepth, dL_dalpha, **kw)
    walk64 = {}
    r64 = backward(o64, scene, cam64, dL_ddepth, dL_dalpha, walk=walk64, **kw)
    r32c = backward(o32c, scene, o32c.convert_camera(ocam), dL_ddepth, dL_dalpha, **kw)
    # the rounding budget of the walk, over the binary32 state the kernels' forward produces bit for bit
    W, H = ocam.width, ocam.height
    st = frame.state(o32, scene, ocam, scale_modifier, sh_deg)
    v, dv = _value(o32, scene, ocam, mode, scale_modifier)
    A, F = o64.render_backward_bound(W, H, np.zeros(3, np.float32), st["ranges"], st["point_list"], st["means"], st["conic"],
                                     st["opacity"], _colour(v), st["final_T"], st["n_contrib"],
                                     _dl3(o32, dL_ddepth, dL_dalpha, H, W))
    A, F = (frame.augment_budget(o64, scene, cam64, st, X, scale_modifier) for X in (A, F))
    Az, Fz = A.copy(), F.copy()
    Az[:, 6:9] = 0.0
    Fz[:, 6:9] = 0.0
    JA, JF = abs_jacobian_apply(o64, scene, cam64, st["radii"], (Az, Fz), scale_modifier, sh_deg)
    front = np.abs(np.asarray(cam64.front[:], np.float64))[None, :]
    adv = np.abs(dv.astype(np.float64))
    JA["pos"] = JA["pos"] + (A[:, 6] * adv)[:, None] * front
    JF["pos"] = JF["pos"] + (F[:, 6] * adv)[:, None] * front
    P = np.asarray(scene["pos"]).reshape(-1, 3).shape[0]
    extra = frame.conditioning(o64, scene, cam64, st["radii"], walk64["go"], scale_modifier, sh_deg)
    B = {}
    for k in KEYS:
        b64 = r64[k].astype(np.float64).reshape(P, -1)
        noise = np.maximum(np.abs(r32[k].astype(np.float64).reshape(P, -1) - b64),
                           np.abs(r32c[k].astype(np.float64).reshape(P, -1) - b64))
        ja, jf = JA[k].reshape(P, -1), JF[k].reshape(P, -1)
        B[k] = GRAD_ROW_K * noise + GRAD_ROW_CU * U32 * ja + jf + GRAD_ROW_FLOOR * ja
        if extra is not None:
            B[k] = B[k] + extra[k].reshape(P, -1)
    return B, r64


def row_bound_with_image(scene, ocam, dL_dimg, dL_ddepth, dL_dalpha, mode="z", bg=(0.0, 0.0, 0.0), scale_modifier=1.0, sh_deg=3):
    """a call that also passes dL_dimg: the sum of the two bounds, against the sum of the two f64 references"""
    Bm, rm = row_bound(scene, ocam, dL_ddepth, dL_dalpha, mode, scale_modifier, sh_deg)
    Bi, ri = gradient_row_bound(scene, ocam, dL_dimg, bg=bg, scale_modifier=scale_modifier, sh_deg=sh_deg)
    P = Bm["pos"].shape[0]
    return ({k: Bm[k] + Bi[k] for k in KEYS},
            {k: rm[k].astype(np.float64).reshape(P, -1) + ri[k].astype(np.float64).reshape(P, -1) for k in KEYS})


def sum_row_bounds(bounds):
    """the bound of a sum of calls (accumulate over views): the sum of their bounds, against the sum of their f64 references"""
    P = bounds[0][0]["pos"].shape[0]
    return ({k: sum(b[0][k] for b in bounds) for k in KEYS},
            {k: sum(b[1][k].astype(np.float64).reshape(P, -1) for b in bounds) for k in KEYS})


def crowd():
    """The crowd: 1500 splats in a tight cloud seen at 45 x 37 -- lists of several rounds, saturated and empty pixels, an image
    that is no multiple of 8.  (scene, pose, W, H)"""
    from conftest import make_scene

    scene = make_scene(np.random.default_rng(5), 1500, spread=0.25, log_scale=(-3.2, 0.5))
    return scene, ([1.6, 0.3, 0.9], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0]), 45, 37
