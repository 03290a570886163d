"""The reference of the caller-supplied feature channels (include/lcgs_hip.h, kernels/features.hip: lcgs_render_features,
lcgs_render_backward_features), composed from the UNCHANGED CPU oracle the way normals_ref.py composes the normal map, and the
per-row bound the kernels' gradients are held to.  No GPU needed.

The oracle composites any 3-column "colour", so a K-channel map is a composition in TRIPLES: columns 3t .. 3t + 2 of the
features, the last triple padded with zero columns (a zero column adds fl(w 0) = 0 to its own channel and nothing to the others).
Forward: the frame's state composited once per triple over a zero background, every operation in o.dtype; the f32 build gives
the kernel's bits (the blend is channel by channel, so the kernel's chunks of 4 / 8 / 16 channels change nothing).
Backward, per oracle build: render_backward per triple with that triple as colour and its 3 planes of dL_dfeature_map; the
walks are linear in (colour, dL), so dL/dmean, dL/dconic and dL/dopacity are summed over the triples and go through the
preprocess-backward once, with a zero colour gradient; each triple's colour-gradient columns are its columns of dL/dfeatures.
The other channels of the same call are normals_ref.backward's (or distortion_ref's, or maps_ref's), added.
Bound: maps_ref.row_bound's formula and constants.  A and F from the f64 walk over the f32 state, summed over the triples;
columns 0-5 go through abs_jacobian_apply, columns 6-8 of each triple bound that triple's dL/dfeatures columns directly (no
Jacobian: the caller's rows are the walk's own output).  The noise term is the f32 and the contracted build's distance from
the f64 build, as there -- sampled in BOTH channel orders (as given, and reversed: four samples for two).  The grouping of K
channels into triples is this file's, not the contract's (the kernel groups by 4 / 8 / 16), so every order is the same
binary32 reference; and two samples under-estimate its own error on needle rows, where the per-splat algebra of the
preprocess-backward turns any change of its inputs' last bits into rounding noise of the size of its cancelling intermediates:
on draw 102 of gpu_util.random_draw (needles and giants) at K = 17 the f32 build itself, composed in other channel orders
(rng seeds 0-3), lands at 0.27, 0.79, 0.35 and 1.59 of the two-sample bound (dL/dscale of row 1154, scale (0.30, 0.005, 0.004),
where 3 x noise is four fifths of the bound), and at 0.20, 0.41, 0.35, 0.49 of the four-sample one; on the crowd and draws
100, 101, 103 the second order changes no worst ratio (tests/test_features_ref.py pins the draw-102 figures).
The gradient dicts and bounds carry one more key, "features" [P, K], which gpu_util.check_gradient_rows holds like any other
attribute."""
import numpy as np

import distortion_ref
import maps_ref
import normals_ref
from gpu_util import GRAD_ROW_CU, GRAD_ROW_FLOOR, GRAD_ROW_K, KEYS, U32, _oracles

MODES = maps_ref.MODES
FKEY = "features"


def noise_orders(K):
    """the channel orders the noise term samples the binary32 builds in: as given, and reversed"""
    return [np.arange(K)] + ([np.arange(K)[::-1]] if K > 1 else [])


def triples(K):
    """[(first column, columns)] of the composition"""
    return [(c, min(3, K - c)) for c in range(0, K, 3)]


def _triple(feats, c, n, dt):
    """columns c .. c + n - 1 as a zero-padded 3-column colour"""
    out = np.zeros((feats.shape[0], 3), dt)
    out[:, :n] = feats[:, c:c + n]
    return out


def _planes(dL, c, n, dt):
    out = np.zeros((3,) + dL.shape[1:], dt)
    out[:n] = dL[c:c + n]
    return out


def compose(o, st, cam, feats):
    """the map [K, H, W] in o.dtype of a forward state `st` (Oracle.forward_state's, or antialias_ref's)"""
    feats = np.asarray(feats, o.dtype)
    K = feats.shape[1]
    out = np.zeros((K, cam.height, cam.width), o.dtype)
    for c, n in triples(K):
        img = normals_ref.compose(o, st, cam, _triple(feats, c, n, o.dtype))
        out[c:c + n] = img[:n]
    return out


def forward(o, scene, cam, feats, scale_modifier=1.0, sh_deg=3):
    """(feature map [K, H, W], forward state) of oracle build `o`"""
    st = o.forward_state(scene, cam, scale_modifier=scale_modifier, sh_deg=sh_deg)
    return compose(o, st, cam, feats), st


def _walks(o, st, cam, feats, dL):
    """(dL/dmean [P, 2], dL/dconic [P, 3], dL/dopacity [P], dL/dfeatures [P, K]) of build `o` over the state `st`"""
    W, H = cam.width, cam.height
    feats, dL = np.asarray(feats, o.dtype), np.asarray(dL, o.dtype)
    K = feats.shape[1]
    assert dL.shape == (K, H, W), (dL.shape, K, H, W)
    gm = gc = go = None
    gf = np.zeros_like(feats)
    for c, n in triples(K):
        m, cn, op, col = o.render_backward(W, H, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"],
                                           st["opacity"], _triple(feats, c, n, o.dtype), st["final_T"], st["n_contrib"],
                                           _planes(dL, c, n, o.dtype))
        gm, gc, go = (m, cn, op) if gm is None else (gm + m, gc + cn, go + op)
        gf[:, c:c + n] = col[:, :n]
    return gm, gc, go, gf


def backward(o, scene, cam, feats, dL_dfmap, dL_dnormal=None, dL_ddist=None, dL_ddepth=None, dL_dalpha=None, mode="z", center=0.0,
             scale_modifier=1.0, sh_deg=3, frame=maps_ref.Classic, walk=None, decide=None):
    """attribute -> gradient of <dL_dfmap, feature_map> + <dL_dnormal, normal> + <dL_ddist, dist> + <dL_ddepth, depth> +
    <dL_dalpha, alpha> in oracle build `o` (its own forward), with "features" [P, K]; walk: a dict that receives the feature
    walks' own dL/dopacity row ("go"); decide: normals_ref's (k, flip)"""
    st = frame.state(o, scene, cam, scale_modifier, sh_deg)
    gm, gc, go, gf = _walks(o, st, cam, feats, dL_dfmap)
    if walk is not None:
        walk["go"] = go
    gc, go = frame.augment(o, st, gc, go)
    g = o.preprocess_backward(scene, cam, st["radii"], gm, gc, np.zeros((gm.shape[0], 3), o.dtype), scale_modifier=scale_modifier,
                              sh_deg=sh_deg)
    g["opacity"] = go
    g["sh"] = np.zeros_like(g["sh"])
    kw = dict(mode=mode, scale_modifier=scale_modifier, sh_deg=sh_deg, frame=frame)
    other = None
    if dL_dnormal is not None:
        other = normals_ref.backward(o, scene, cam, dL_dnormal, dL_ddist, dL_ddepth, dL_dalpha, center=center, decide=decide, **kw)
    elif dL_ddist is not None:
        other = distortion_ref.backward(o, scene, cam, dL_ddist, dL_ddepth, dL_dalpha, center=center, **kw)
    elif dL_ddepth is not None or dL_dalpha is not None:
        other = maps_ref.backward(o, scene, cam, dL_ddepth, dL_dalpha, **kw)
    if other is not None:
        g = {key: g[key] + other[key] for key in g}
    g[FKEY] = gf
    return g


def row_bound(scene, ocam, feats, dL_dfmap, scale_modifier=1.0, sh_deg=3, frame=maps_ref.Classic, orders=None):
    """(per attribute [P, n] bound, f64 reference), "features" [P, K] among the attributes, for a features backward without any
    other incoming gradient.  Another channel of the same call is added with sum_row_bounds.  orders: the channel orders the
    noise term is sampled in (default noise_orders(K); tests/test_features_ref.py passes the given order alone)."""
    from oracle import abs_jacobian_apply

    o32, o64, o32c = _oracles()
    ocam = o32.convert_camera(ocam)
    cam64 = o64.convert_camera(ocam)
    feats32 = np.asarray(feats, np.float32)
    dL32 = np.asarray(dL_dfmap, np.float32)
    K = feats32.shape[1]
    kw = dict(scale_modifier=scale_modifier, sh_deg=sh_deg, frame=frame)
    walk64 = {}
    r64 = backward(o64, scene, cam64, feats32, dL32, walk=walk64, **kw)
    # the binary32 samples of the noise term: the f32 and the contracted build, each composed in both channel orders
    samples = []
    for order in (orders if orders is not None else noise_orders(K)):
        back = np.argsort(order)
        for o, cam in ((o32, ocam), (o32c, o32c.convert_camera(ocam))):
            g = backward(o, scene, cam, feats32[:, order], dL32[order], **kw)
            g[FKEY] = g[FKEY][:, back]
            samples.append(g)
    # the rounding budget of the walks, over the binary32 state the kernels' forward produces bit for bit
    W, H = ocam.width, ocam.height
    st = frame.state(o32, scene, ocam, scale_modifier, sh_deg)
    P = feats32.shape[0]
    A, F = np.zeros((P, 9)), np.zeros((P, 9))
    Af, Ff = np.zeros((P, K)), np.zeros((P, K))
    for c, n in triples(K):
        a, f = o64.render_backward_bound(W, H, np.zeros(3, np.float32), st["ranges"], st["point_list"], st["means"], st["conic"],
                                         st["opacity"], _triple(feats32, c, n, np.float32), st["final_T"], st["n_contrib"],
                                         _planes(dL32, c, n, np.float32))
        A[:, 0:6] += a[:, 0:6]
        F[:, 0:6] += f[:, 0:6]
        Af[:, c:c + n] = a[:, 6:6 + n]
        Ff[:, c:c + n] = f[:, 6:6 + n]
    A, F = (frame.augment_budget(o64, scene, cam64, st, X, scale_modifier) for X in (A, F))
    JA, JF = abs_jacobian_apply(o64, scene, cam64, st["radii"], (A, F), scale_modifier, sh_deg)
    JA[FKEY], JF[FKEY] = Af, Ff
    extra = frame.conditioning(o64, scene, cam64, st["radii"], walk64["go"], scale_modifier, sh_deg)
    B, R = {}, {}
    for key in KEYS + (FKEY,):
        b64 = r64[key].astype(np.float64).reshape(P, -1)
        noise = np.max([np.abs(g[key].astype(np.float64).reshape(P, -1) - b64) for g in samples], axis=0)
        ja, jf = JA[key].reshape(P, -1), JF[key].reshape(P, -1)
        B[key] = GRAD_ROW_K * noise + GRAD_ROW_CU * U32 * ja + jf + GRAD_ROW_FLOOR * ja
        if extra is not None and key in extra:
            B[key] = B[key] + extra[key].reshape(P, -1)
        R[key] = b64
    return B, R


def sum_row_bounds(bounds):
    """maps_ref.sum_row_bounds with the "features" attribute carried along: the bound of a sum of calls or channels is the sum
    of their bounds, against the sum of their f64 references (a term without feature rows adds nothing to them)"""
    B, R = maps_ref.sum_row_bounds(bounds)
    fb = [b for b in bounds if FKEY in b[0]]
    if fb:
        B[FKEY] = sum(b[0][FKEY] for b in fb)
        R[FKEY] = sum(np.asarray(b[1][FKEY], np.float64) for b in fb)
    return B, R


def geometry_only(bound):
    """a bound without its "features" attribute: a call that passes d_dL_dfeatures NULL"""
    return tuple({k: v for k, v in d.items() if k != FKEY} for d in bound)
