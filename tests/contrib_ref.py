"""The reference of the per-splat blend-weight statistics (include/lcgs_hip.h lcgs_contrib_accumulate, kernels/contrib.hip),
composed from the UNCHANGED f32 CPU oracle the way maps_ref.py composes the maps.  No GPU needed.

The frame's kept state is composited once more over a zero background with ONE-HOT colours: one splat gets 1 in channel c,
every other splat on the pixel's list 0.  A splat appears at most once in a pixel's sequence and every other term is w * 0, so channel c of that
image holds the splat's w = T alpha at every pixel, bit for bit, in the renderer's own binary32 expressions.  Then
    weight_max = the channel's max          pixels = its positive entries (w >= 1e-4 / 255 > 0 whenever blended)
    weight_sum's reference = the channel's sum in float64 (the terms are exact; only the order of a binary32 sum is free)
Rows on no list are never rendered: they stay zero."""
import numpy as np

U32 = 2.0 ** -24
POSE2 = ([-1.2, 1.1, 0.7], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0])  # the crowd's second view


def _pack(tiles_of_row, G):
    """rows -> groups whose members share no tile (first fit, rows with many tiles first): the members of a group can wear the
    same colour, because a pixel's list holds at most one of them"""
    order = sorted(tiles_of_row, key=lambda r: -len(tiles_of_row[r]))
    occ, groups = np.zeros((0, G), bool), []
    for r in order:
        t = tiles_of_row[r]
        free = np.nonzero(~occ[:, t].any(axis=1))[0]
        if free.size == 0:
            occ = np.concatenate([occ, np.zeros((1, G), bool)])
            groups.append([])
            g = len(groups) - 1
        else:
            g = int(free[0])
        occ[g, t] = True
        groups[g].append(r)
    return groups


def view_stats(o, scene, cam, scale_modifier=1.0, sh_deg=3):
    """dict(weight_sum f64 [P], weight_max f32 [P], pixels u32 [P], tiles u32 [P] (16x16 tiles in which a pixel blended the
    row), listed (rows on some list), total f64 [H, W] (sum over the rows of w), state) of one view in oracle build `o` (f32).
    Rows that share no tile share a colour (a pixel's list holds one of them at most, so its channel is still one splat's w
    and exact zeros); each is read back from the pixels of its own tiles."""
    st = o.forward_state(scene, cam, scale_modifier=scale_modifier, sh_deg=sh_deg)
    W, H = cam.width, cam.height
    P = np.asarray(scene["pos"]).reshape(-1, 3).shape[0]
    out = {"weight_sum": np.zeros(P, np.float64), "weight_max": np.zeros(P, np.float32), "pixels": np.zeros(P, np.uint32),
           "tiles": np.zeros(P, np.uint32), "total": np.zeros((H, W), np.float64), "state": st}
    gx = (W + 15) // 16
    tiles_of_row = {}
    for t, (a, b) in enumerate(st["ranges"]):
        rows = st["point_list"][a:b]
        assert np.unique(rows).size == rows.size  # a splat appears at most once in a tile's list
        for r in rows:
            tiles_of_row.setdefault(int(r), []).append(t)
    out["listed"] = np.array(sorted(tiles_of_row), np.int64)
    groups = _pack(tiles_of_row, st["ranges"].shape[0])
    for k in range(0, len(groups), 3):
        col = np.zeros((P, 3), o.dtype)
        for c, rows in enumerate(groups[k:k + 3]):
            col[rows, c] = 1
        img = o.render_forward(W, H, np.zeros(3), st["ranges"], st["point_list"], st["means"], st["conic"], st["opacity"], col)[0]
        assert img.dtype == np.float32 and not (img < 0).any()
        out["total"] += img.astype(np.float64).sum(axis=0)
        for c, rows in enumerate(groups[k:k + 3]):
            for r in rows:
                blocks = [img[c, 16 * (t // gx):16 * (t // gx) + 16, 16 * (t % gx):16 * (t % gx) + 16] for t in tiles_of_row[r]]
                out["weight_max"][r] = max(b.max() for b in blocks)
                out["pixels"][r] = sum(int((b > 0).sum()) for b in blocks)
                out["weight_sum"][r] = sum(b.astype(np.float64).sum() for b in blocks)
                out["tiles"][r] = sum(bool((b > 0).any()) for b in blocks)
    return out


def accumulate(views):
    """the statistics over several views (view_stats results): sums and counts add, the max is the max, `views` counts the
    views in which some pixel blended the row"""
    acc = {"weight_sum": sum(v["weight_sum"] for v in views), "weight_max": np.maximum.reduce([v["weight_max"] for v in views]),
           "pixels": sum(v["pixels"].astype(np.uint32) for v in views).astype(np.uint32),
           "views": sum((v["pixels"] > 0).astype(np.uint32) for v in views).astype(np.uint32)}
    return acc


def sum_bound(ref_sum, pixels):
    """|binary32 sum in ANY order - exact sum| <= gamma_n x exact sum for n non-negative terms (Higham, Accuracy and Stability of
    Numerical Algorithms, section 4.2): gamma_n = n u / (1 - n u), u = 2^-24"""
    n = pixels.astype(np.float64)
    return n * U32 / (1.0 - n * U32) * ref_sum


def keep_predicate(stats, min_weight_max=0.0, min_weight_sum=0.0, min_pixels=0, min_views=0):
    """lcgs_prune_config's rule on binary32 / uint32 statistics: every enabled (non-zero) minimum is met"""
    P = next(iter(stats.values())).shape[0]
    keep = np.ones(P, bool)
    if min_weight_max != 0:
        keep &= stats["weight_max"].astype(np.float32) >= np.float32(min_weight_max)
    if min_weight_sum != 0:
        keep &= stats["weight_sum"].astype(np.float32) >= np.float32(min_weight_sum)
    if min_pixels != 0:
        keep &= stats["pixels"].astype(np.uint64) >= np.uint64(min_pixels)
    if min_views != 0:
        keep &= stats["views"].astype(np.uint64) >= np.uint64(min_views)
    return keep


def sub_scene(scene, keep):
    return {k: np.ascontiguousarray(np.asarray(scene[k])[keep]) for k in ("pos", "scale", "rotq", "sh", "opacity")}


def crowd_views(oracle):
    """the crowd (maps_ref.crowd) from its own pose and from POSE2: (scene, W, H, [(pose, oracle camera, view_stats)] x 2)"""
    import maps_ref

    scene, pose, W, H = maps_ref.crowd()
    views = []
    for p in (pose, POSE2):
        cam = oracle.lookat(*p, width=W, height=H)
        views.append((p, cam, view_stats(oracle, scene, cam)))
    return scene, W, H, views
