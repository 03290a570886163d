"""`-m gpu`: the splat-ownership backward held to the per-row bound (gpu_util.check_gradient_rows, unchanged), through the
Python binding and the C ABI only -- the one backward tests/test_gpu_owner.py holds by a norm per attribute.

  A  the two halves (owner_project / owner_render / owner_render_backward / owner_backward), route by route: the Jacobian
     kernel with shifted bases, the STAGED SH copy of k_preprocess_backward (no other caller reaches it), the lane-wise rows
     of an unaligned dL_dsh and of degrees 0 .. 2; one, two and three owners at boundaries that are multiples of neither 4
     nor 64; an owner that sees nothing and one that sees all of its span; on-screen counts at wave and block boundaries
     inside one owner's span; two views accumulated; a context-owned, re-ordered scene;
  B  the step with its transport (Comm.owner_step_forward / _backward / owner_step): world size 1 over RCCL, 2 and 3
     in-process ranks over the loopback group, synchronous and without read-back, padded segments that are really padded,
     the step that is repeated because a message was clipped.

Every gradient array starts at 7.0; rows outside the range(s) written must keep it, rows of a written range that no view
sees must be exact zeros, every other row of every attribute lies within its bound (a sum of views: the sum of the views'
bounds against the sum of their f64 references), and every frame is the oracle's bit for bit.  Each case first asserts on
the oracle that its scene is what it claims (the `*_premise` functions need no GPU: tests/test_owner_rows_premises.py runs
them on the CPU), and each (scene, pose, dL/dimg) computes its oracle frame and its bound once (gpu_util.View)."""
import threading

import numpy as np
import pytest
import torch

import luisacomputegaussiansplatting_amd as L
from conftest import make_scene
from gpu_util import BG, DEV, KEYS, View, assert_image_parity, cached, check_gradient_rows, dev, sevens, sum_bounds

pytestmark = pytest.mark.gpu
POSE = ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1])
POSE2 = ([2.5, 1.5, 1.0], [0, 0, 0.5], [0, 0, 1])
POSE3 = ([0.5, -3.2, 1.5], [0, 0, 0.5], [0, 0, 1])
FAR = ([97, 99.5, 102.3], [100, 100, 100.5], [0, 0, 1])     # POSE moved by +100: sees the rows parked there, and only them
NOWHERE = ([500, 500, 500], [600, 500, 500], [0, 0, 1])     # sees nothing at all
W, H = 200, 150
FILL = 7.0


def _mask(P, spans):
    m = np.zeros(P, bool)
    for f, c in spans:
        m[f:f + c] = True
    return m


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _check_rows(g, views, spans, tag, perm=None):
    """g (the context's row order; row r = file row perm[r]) after `views` were written into `spans`: rows outside the spans
    keep the fill, rows of the spans no view sees are exact zeros, every row of the spans is within the (summed) bound"""
    P = views[0].P
    bound = views[0].bound() if len(views) == 1 else sum_bounds(views)
    flat = {k: _np(g[k]).reshape(P, -1) for k in KEYS}
    cov = _mask(P, spans)
    idx = np.nonzero(cov)[0]
    seen = np.zeros(P, bool)
    for v in views:
        seen |= v.on
    if perm is not None:
        seen = seen[perm]
    for k in KEYS:
        assert (flat[k][~cov] == FILL).all(), (tag, k, "a row outside the ranges written lost its fill")
        assert not flat[k][cov & ~seen].any(), (tag, k, "a row of a written range that no view sees is not an exact zero")
    return check_gradient_rows({k: flat[k][idx] for k in KEYS}, None, None, None, bound=bound,
                               rows=perm[idx] if perm is not None else idx, tag=tag)


def _renderer(scene, deg=3):
    r = L.Renderer(L.Context(0))
    d = {k: dev(scene[k]) for k in KEYS}
    r.bind_scene(*[d[k] for k in KEYS], sh_degree=deg)
    assert d["sh"].data_ptr() % 16 == 0
    r._scene_keepalive = d
    return r


# ---------------------------------------------------------------------------------------- A: the two halves, route by route
P_A, HEAD, TAIL = 4001, 53, 137         # rows [0, HEAD) and [P - TAIL, P) belong to no span and are parked where no view looks
F0, F1, W1 = 1501, 2107, 2177           # [F0, F1): parked at +100, seen from FAR only; [F1, W1): in front of the cloud, all seen
END = P_A - TAIL
SPANS = {"one": [(HEAD, END - HEAD)],
         "two": [(HEAD, F0 - HEAD), (F0, END - F0)],
         "three_one_unseen": [(HEAD, F0 - HEAD), (F0, F1 - F0), (F1, END - F1)],
         "three_one_all_seen": [(HEAD, F1 - HEAD), (F1, W1 - F1), (W1, END - W1)]}
ROUTES = ("jacobian", "staged", "unaligned")
HALVES_POSES = {"near": (POSE, 20), "near2": (POSE2, 21), "far": (FAR, 22)}


def halves_scene(deg):
    def make():
        rng = np.random.default_rng(500)
        scene = make_scene(rng, P_A)
        scene["pos"][:HEAD, 2] += 300.0   # straight up: behind every camera of this file
        scene["pos"][END:, 2] += 300.0
        scene["pos"][F0:F1] += 100.0
        eye, at = np.array(POSE[0], np.float64), np.array(POSE[1], np.float64)
        d = (at - eye) / np.linalg.norm(at - eye)
        scene["pos"][F1:W1] = (eye + 1.7 * d + rng.uniform(-0.3, 0.3, (W1 - F1, 3))).astype(np.float32)
        scene["scale"][F1:W1], scene["opacity"][F1:W1] = 0.02, 0.6
        scene["sh"] = np.ascontiguousarray(scene["sh"][:, :(deg + 1) ** 2 * 3])
        return scene
    return cached(("own A scene", deg), make)


def halves_premise(oracle, name="near", deg=3):
    """P = 4001 at 200 x 150.  near / near2 see the cloud, nothing of [0, 53), [3864, 4001) (no span covers them) and nothing
    of [1501, 2107) (parked at +100); near sees and hits EVERY row of [2107, 2177); far sees rows of [1501, 2107) only."""
    def make():
        pose, seed = HALVES_POSES[name]
        return View(oracle, halves_scene(deg), pose, W, H, seed=seed, sh_deg=deg)
    v = cached(("own A", name, deg), make)
    assert not v.on[:HEAD].any() and not v.on[END:].any()
    if name == "far":
        assert not v.on[:F0].any() and not v.on[F1:].any() and v.hit[F0:F1].sum() >= 300, int(v.hit[F0:F1].sum())
    else:
        assert not v.on[F0:F1].any() and v.hit[HEAD:F0].sum() >= 1000 and v.hit[W1:END].sum() >= 1000
        assert name != "near" or (v.on[F1:W1].all() and v.hit[F1:W1].all())
    # boundaries that are multiples of neither 4 nor 64, in rows and in floats of the 3-wide arrays
    assert all(f % 4 and f % 64 and (3 * f) % 4 for f in (HEAD, F0, F1, W1))
    return v


def _halves(r, v, spans, g, route, slot0=0, accumulate=False, perm=None):
    """one view through the two halves into g; returns the rows each span projected.  route "jacobian": owner_project keeps
    the colour Jacobian; "staged" / "unaligned" / low degrees: owner_project(keep_state=False), owner_render(keep_state=True)"""
    cam, P = v.cam(), v.P
    parts = []
    for o, (f, c) in enumerate(spans):
        rows, recs = r.owner_project(slot0 + o, cam, f, c, keep_state=route == "jacobian")
        got = rows.cpu().numpy().astype(np.int64)
        assert (got[1:] > got[:-1]).all() and ((got >= f) & (got < f + c)).all(), (o, f, c)
        span = _mask(P, [(f, c)])
        m = np.zeros(P, bool)
        m[got] = True
        on, hit = (v.on, v.hit) if perm is None else (v.on[perm], v.hit[perm])
        assert not (m & ~on).any() and not (hit & span & ~m).any(), (o, int(m.sum()), int((on & span).sum()), int((hit & span).sum()))
        parts.append((rows, recs))
    rows, recs = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    assert rows.shape[0] > 0
    img = torch.full((3, v.H, v.W), -1.0, device=DEV)
    r.owner_render(cam, rows, recs, img, bg=v.bg, keep_state=True)
    g2d = torch.zeros(rows.shape[0], r.OWNER_GRAD_FLOATS, device=DEV)
    r.owner_render_backward(dev(v.dL), g2d)
    at = 0
    for o, (rows_o, _) in enumerate(parts):
        n = int(rows_o.shape[0])
        r.owner_backward(slot0 + o, g2d[at:at + n].contiguous(), *[g[k] for k in KEYS], accumulate=accumulate)
        at += n
    r.ctx.synchronize()
    assert_image_parity(img.cpu().numpy(), v.ref)
    return [int(p[0].shape[0]) for p in parts]


def _grads_for(scene, route):
    g = sevens(scene, sh_offset=1 if route == "unaligned" else 0)
    assert g["sh"].data_ptr() % 16 == (4 if route == "unaligned" else 0)
    return g


@pytest.mark.parametrize("route", ROUTES)
def test_which_kernel_runs(lcgs, oracle, route):
    """Two owners, degree 3.  The kernel cannot be observed through the ABI; the premise rests on these lines:
    project_rows (abi_owner.cpp): `s.has_jac = keep_state && build_records_writes_jacobian(...)`, and owner_backward_rows hands
    `s.has_jac ? s.shjac : nullptr` to launch_preprocess_backward (backward.hip), which takes k_preprocess_backward_jac only
    `if (shjac && sh_deg == 3 && dL_dsh 16-byte aligned)`; in k_preprocess_backward, `staged = sh_deg == 3 && sh aligned &&
    dL_dsh aligned`.  The bases are shifted by 192 bytes a row, so an aligned array stays aligned at every row_first.
      jacobian   keep_state=True                         -> k_preprocess_backward_jac, bases shifted by row_first
      staged     owner_project(keep_state=False)         -> k_preprocess_backward, staged: both LDS halves, 12 lanes a row
      unaligned  the same, dL_dsh one float further      -> k_preprocess_backward, lane-wise degree-3 rows"""
    v = halves_premise(oracle)
    r, g = _renderer(v.scene), _grads_for(v.scene, route)
    _halves(r, v, SPANS["two"], g, route)
    _check_rows(g, [v], SPANS["two"], f"A1 {route}")


@pytest.mark.parametrize("deg", [0, 1, 2])
def test_low_degrees_write_lane_wise_rows(lcgs, oracle, deg):
    """feat * row_first = 3, 12, 27 floats a row: no Jacobian is kept below degree 3 (build_records_writes_jacobian), so
    either keep_state reaches k_preprocess_backward's lane-wise rows; both are run"""
    v = halves_premise(oracle, deg=deg)
    assert v.scene["sh"].shape[1] == (3, 12, 27)[deg]
    r = _renderer(v.scene, deg)
    for route in ("jacobian", "staged"):
        g = _grads_for(v.scene, route)
        _halves(r, v, SPANS["two"], g, route)
        _check_rows(g, [v], SPANS["two"], f"A1d degree {deg}, keep_state={route == 'jacobian'}")


@pytest.mark.parametrize("route", ["jacobian", "staged"])
@pytest.mark.parametrize("spans", ["one", "three_one_unseen", "three_one_all_seen"])
def test_spans(lcgs, oracle, spans, route):
    """one owner; three owners of whom the middle one sees nothing (an empty g2d: its span must be exact zeros) or all of its
    span (every row projected)"""
    v = halves_premise(oracle)
    r, g = _renderer(v.scene), _grads_for(v.scene, route)
    counts = _halves(r, v, SPANS[spans], g, route)
    if spans == "three_one_unseen":
        assert counts[1] == 0
        assert all(not g[k][F0:F1].any() for k in KEYS)
    if spans == "three_one_all_seen":
        assert counts[1] == W1 - F1
    _check_rows(g, [v], SPANS[spans], f"A2 {spans} {route}")


BOUNDARY_V = (1, 63, 64, 65, 255, 256, 257)
INNER = (131, 600)
BOUNDARY_SPANS = [(0, INNER[0]), INNER, (INNER[0] + INNER[1], 1000 - INNER[0] - INNER[1])]


def boundary_premise(oracle, V):
    """the recipe of test_gpu_backward_paths.boundary_premise (P = 1000 at 96 x 80) with the count fixed inside an INNER range
    only: of rows [131, 731) exactly V are on screen (on == hit), every other row of the range is parked; the rows before and
    after it stay, on screen, and belong to two further owners"""
    def make():
        rng = np.random.default_rng(400)
        scene = make_scene(rng, 1000, spread=0.25, log_scale=(-3.5, 0.7))
        a, b = INNER[0], INNER[0] + INNER[1]
        shown = np.nonzero(View(oracle, dict(scene), POSE, 96, 80, seed=8).hit[a:b])[0] + a
        assert shown.size >= V, shown.size
        keep = np.sort(rng.choice(shown, V, replace=False))
        off = _mask(1000, [INNER])
        off[keep] = False
        scene["pos"][off] += 100.0
        v = View(oracle, scene, POSE, 96, 80, seed=8)
        assert np.array_equal(np.nonzero(v.on[a:b])[0] + a, keep) and np.array_equal(v.hit[a:b], v.on[a:b])
        assert v.hit[:a].sum() >= 50 and v.hit[b:].sum() >= 50 and a % 64 and a % 4
        return v
    return cached(("own A3", V), make)


@pytest.mark.parametrize("route", ["jacobian", "staged"])
@pytest.mark.parametrize("V", BOUNDARY_V)
def test_counts_at_wave_and_block_boundaries_inside_a_span(lcgs, oracle, V, route):
    """`slot < nvalid` of the cooperative SH load and store matters in a partly filled wave only; row_first = 131"""
    v = boundary_premise(oracle, V)
    r, g = _renderer(v.scene), _grads_for(v.scene, route)
    counts = _halves(r, v, BOUNDARY_SPANS, g, route)
    assert counts[1] == V, counts
    _check_rows(g, [v], BOUNDARY_SPANS, f"A3 V={V} {route}")


@pytest.mark.parametrize("route", ["jacobian", "staged"])
@pytest.mark.parametrize("case", ["both_see_the_cloud", "second_view_only", "first_view_misses_a_span"])
def test_two_views_accumulate(lcgs, oracle, case, route):
    """view 1 into slots 0.., view 2 into the next slots with accumulate=True, held to the sum of the two bounds.
    second_view_only: rows [1501, 2107) of the second owner are on screen in view 2 alone -- the add lands on the zero view
    1's clear left.  first_view_misses_a_span: view 1 sees nothing of the middle owner -- its owner_backward returns behind the clear."""
    v1 = halves_premise(oracle)
    v2 = halves_premise(oracle, "near2" if case == "both_see_the_cloud" else "far")
    spans = SPANS["three_one_unseen" if case == "first_view_misses_a_span" else "two"]
    r, g = _renderer(v1.scene), _grads_for(v1.scene, route)
    c1 = _halves(r, v1, spans, g, route)
    _check_rows(g, [v1], spans, f"A4 {case} {route}, view 1")
    c2 = _halves(r, v2, spans, g, route, slot0=len(spans), accumulate=True)
    if case == "first_view_misses_a_span":
        assert c1[1] == 0 and c2[1] > 0 and c2[0] == c2[2] == 0
    if case == "second_view_only":
        assert c2[0] == 0 and c2[1] > 0
    _check_rows(g, [v1, v2], spans, f"A4 {case} {route}, two views")


def test_a_reordered_scene(lcgs, oracle):
    """upload_scene: the context keeps the scene along a Morton curve; two owners of the RE-ORDERED rows (row r = file row
    permutation()[r]), the Jacobian route"""
    v = halves_premise(oracle)
    r = L.Renderer(L.Context(0))
    r.upload_scene(v.scene)
    perm = r.permutation().cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(v.P)) and not np.array_equal(perm, np.arange(v.P))
    spans = [(0, 1999), (1999, v.P - 1999)]
    g = sevens(v.scene)
    _halves(r, v, spans, g, "jacobian", perm=perm)
    _check_rows(g, [v], spans, "A5 re-ordered", perm=perm)


# ---------------------------------------------------------------------------------------- B: the step with its transport
def _padded(n, count):
    return min(count, n + n // 4 + 1024)  # comm_owner.cpp padded_rows


def _ranges(P, world):
    c = P // world  # lcgs_comm_owner_rows
    return [(c * r, c if r < world - 1 else P - c * r) for r in range(world)]


def _table(views, on=None):
    """table[o][v]: rows of owner o's range among view v's `on` rows"""
    P, N = views[0].P, len(views)
    return [[int((views[v].on if on is None else on[v])[f:f + c].sum()) for v in range(N)] for f, c in _ranges(P, N)]


def _offset_sevens(scene, off):
    """gradient arrays of 7.0; off: pos, scale, sh and opacity start one float past a 16-byte boundary (rotq must be aligned)"""
    g = {}
    for k in KEYS:
        n = scene[k].size
        flat = torch.full((n + 4,), FILL, device=DEV)
        o = 1 if off and k != "rotq" else 0
        g[k] = flat[o:o + n].view(scene[k].shape)
        assert g[k].data_ptr() % 16 == 4 * o
    return g


def _fill_edges(g, first, count):
    """per array: (head, tail) floats of the DenseFill side job of k_render_backward (LCGS_FILL, backward.hip)"""
    out = {}
    for k in KEYS:
        w = g[k][0].numel() if g[k].dim() > 1 else 1
        base, n = g[k].data_ptr() + 4 * w * first, w * count
        head = min(((16 - base % 16) % 16) // 4, n)
        out[k] = (head, (n - head) % 4)
    return out


def _steps(scene, world, steps, async_steps, loopback=True, offset=False):
    """`world` ranks (one host thread and side stream each over the loopback group; one rank over RCCL in this thread) run
    `steps` = [views of the step]; every array is refilled with 7.0 before each step and read after it.
    -> per rank: [{img, g, stats, redo}] per step, and the rank's (head, tail) of the five fill bases"""
    group = L.api.LoopbackGroup(world) if loopback else None
    out, errors = [None] * world, []
    first_count = _ranges(steps[0][0].P, world)

    def rank_main(me, side):
        r = L.Renderer(L.Context(0, side.cuda_stream) if side is not None else L.Context(0))
        d = {k: dev(scene[k]) for k in KEYS}
        r.bind_scene(*[d[k] for k in KEYS])
        comm = L.Comm(r.ctx, me, world, loopback=group) if loopback else L.Comm(r.ctx, 0, 1)
        try:
            if async_steps:
                comm.owner_step_set_async(True)
            g, snaps = _offset_sevens(scene, offset), []
            for views in steps:
                cams, me_view = [v.cam() for v in views], views[me]
                for k in KEYS:
                    g[k].fill_(FILL)
                img = torch.full((3, me_view.H, me_view.W), -1.0, device=DEV)
                redo = None
                if async_steps:
                    redo = comm.owner_step(cams, img, dev(me_view.dL), g, bg=me_view.bg)
                else:
                    comm.owner_step_forward(cams, img, bg=me_view.bg)
                    comm.owner_step_backward(dev(me_view.dL), g)
                r.ctx.synchronize()
                if side is not None:
                    side.synchronize()
                snaps.append({"img": img.cpu().numpy(), "g": {k: g[k].cpu().numpy() for k in KEYS}, "stats": comm.stats(), "redo": redo})
            out[me] = (snaps, _fill_edges(g, *first_count[me]))
        finally:
            comm.close()

    def thread_main(me):
        try:
            side = torch.cuda.Stream(device=DEV)
            with torch.cuda.stream(side):
                rank_main(me, side)
        except Exception as e:  # noqa: BLE001
            errors.append((me, repr(e)))

    torch.cuda.synchronize()
    if not loopback:
        rank_main(0, None)
        return out
    threads = [threading.Thread(target=thread_main, args=(me,)) for me in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    assert all(not t.is_alive() for t in threads), "a rank hangs"
    group.close()
    return out


def _check_step(snap, views, me, tag, first_step=True, async_steps=False):
    """rank me's frame is its view's, its range holds the sum of the views, everything else keeps the fill"""
    v, world = views[me], len(views)
    if v.ref["num_rendered"] == 0:
        # nothing on this rank's screen: a step that read its sizes back leaves the image alone (lcgs_owner_render, as the
        # reference does); one that did not draws the empty padded segments: the background
        bgimg = np.broadcast_to(np.array(v.bg, np.float32)[:, None, None], snap["img"].shape)
        assert (snap["img"] == -1.0).all() or (async_steps and not first_step and np.array_equal(snap["img"], bgimg))
    else:
        assert_image_parity(snap["img"], v.ref)
    return _check_rows(snap["g"], views, [_ranges(v.P, world)[me]], tag)


def _check_all(out, steps, tag, async_steps):
    for me, (snaps, _) in enumerate(out):
        for s, (snap, views) in enumerate(zip(snaps, steps)):
            _check_step(snap, views, me, f"{tag} rank {me} step {s}", s == 0, async_steps)


@pytest.mark.parametrize("self_p2p", [False, True], ids=["own_share_copied", "self_p2p"])
@pytest.mark.parametrize("async_steps", [False, True], ids=["sync", "async"])
def test_step_at_world_size_one_over_rccl(lcgs, oracle, monkeypatch, async_steps, self_p2p):
    """the scene of A (P = 4001), one rank owning [0, P).  Without read-back and without self-p2p, steps 2 and 3 read the
    rank's own projection where it lies and its 2-D gradients from the aliased g2d_all; checked after every step"""
    if self_p2p:
        monkeypatch.setenv("LCGS_OWNER_SELF_P2P", "1")
    v = halves_premise(oracle)
    steps = [[v]] * 3
    out = _steps(v.scene, 1, steps, async_steps, loopback=False)
    _check_all(out, steps, f"B1 {'async' if async_steps else 'sync'} self_p2p={self_p2p}", async_steps)
    snaps = out[0][0]
    n = snaps[0]["stats"]["touched_rows"]
    assert int(v.hit.sum()) <= n <= v.V and all(s["stats"]["touched_rows"] == n for s in snaps)
    for s, snap in enumerate(snaps):
        rows = _padded(n, v.P) if async_steps and s > 0 else n  # (steps 2, 3 of async ran without read-back: padded messages)
        want = rows * (4 + 48 + 48) if self_p2p else 0
        assert snap["stats"]["bytes_sent"] == want == snap["stats"]["bytes_received"], (s, snap["stats"], want)
        assert snap["redo"] in (None, 0)


def ranks_premise(oracle, world):
    """P = 6001 (2 ranks) / 9001 (3 ranks), ranges of 3000 (+1) rows.  Asserted on the `on` sets:
      * one rank's view sees nothing at all (n_all == 0: no fill, mode 0 for its view-0 slot);
      * one rank whose own view is not empty (the fill runs) holds nothing on view 0 but rows on a later view (mode 2 returns
        early, the first add lands on what the fill cleared);
      * one (owner, view) pair is empty while another pair of that owner is not.
    2 ranks: views (NOWHERE, FAR); [0, 1500) the cloud, [1500, 6001) parked at +100.
    3 ranks: views (POSE, FAR, NOWHERE); [0, 1500) and [6000, 9001) the cloud, [1500, 6000) parked at +100."""
    def make():
        P = {2: 6001, 3: 9001}[world]
        scene = make_scene(np.random.default_rng(600 + world), P)
        scene["pos"][1500:6000 if world == 3 else P] += 100.0
        poses = (NOWHERE, FAR) if world == 2 else (POSE, FAR, NOWHERE)
        return [View(oracle, scene, p, W, H, seed=30 + i) for i, p in enumerate(poses)]
    views = cached(("own B2", world), make)
    for rows in ([v.on for v in views], [v.hit for v in views]):
        t = _table(views, rows)
        n_all = [sum(t[o][v] for o in range(world)) for v in range(world)]
        assert any(n == 0 for n in n_all), n_all
        assert any(n_all[o] > 0 and t[o][0] == 0 and any(t[o][1:]) for o in range(world)), t
        assert any(0 in t[o] and any(t[o]) for o in range(world)), t
    assert any(v.ref["num_rendered"] == 0 for v in views)
    return views


@pytest.mark.parametrize("async_steps", [False, True], ids=["sync", "async"])
@pytest.mark.parametrize("world", [2, 3])
def test_step_with_ranks_in_process(lcgs, oracle, world, async_steps):
    """synchronous: two steps on aligned arrays; without read-back: three steps on arrays that start one float past a 16-byte
    boundary.  The fill's heads and tails: at least one rank has a non-empty head or tail on pos, scale, sh and opacity in
    one of the two variants (dL_drotq must be 16-byte aligned and its rows are 16 bytes: it never has either; with aligned
    arrays and row_first = 3000 the last rank's 3001 rows leave tails on pos, scale and opacity only)."""
    views = ranks_premise(oracle, world)
    steps = [views] * (3 if async_steps else 2)
    out = _steps(views[0].scene, world, steps, async_steps, offset=async_steps)
    edges = [e for _, e in out]
    for k in ("pos", "scale", "opacity") + (("sh",) if async_steps else ()):
        assert any(e[k] != (0, 0) for e in edges), (k, edges)
    if async_steps:
        assert any(all(e[k][0] for k in ("pos", "scale", "sh", "opacity")) for e in edges), edges
    _check_all(out, steps, f"B2 world {world} {'async' if async_steps else 'sync'}", async_steps)
    assert all(s["redo"] in (None, 0) for snaps, _ in out for s in snaps)


PAD_POSES = (POSE, POSE2, POSE3)


def padding_premise(oracle):
    """P = 12 000, three ranks of 4000 rows: the second half of every range is parked where no view looks, so every (owner,
    view) has n <= 2000 on-screen rows and n + n // 4 + 1024 < 4000 -- every padded segment is longer than its rows and
    shorter than the range, and every view's padded total is below P (or the step falls back to read-back)"""
    def make():
        scene = make_scene(np.random.default_rng(700), 12000)
        for o in range(3):
            scene["pos"][o * 4000 + 2000:(o + 1) * 4000, 2] += 300.0
        return [View(oracle, scene, p, W, H, seed=40 + i) for i, p in enumerate(PAD_POSES)]
    views = cached("own B3", make)
    t = _table(views)
    ranges = _ranges(12000, 3)
    assert ranges == [(0, 4000), (4000, 4000), (8000, 4000)]
    for o in range(3):
        for v in range(3):
            assert 0 < t[o][v] and t[o][v] + t[o][v] // 4 + 1024 < 4000, t
        assert not any(view.on[o * 4000 + 2000:(o + 1) * 4000].any() for view in views)
    assert all(sum(_padded(t[o][v], 4000) for o in range(3)) <= 12000 for v in range(3))
    assert all(int(view.hit[o * 4000:o * 4000 + 2000].sum()) > 0 for view in views for o in range(3))
    return views


def test_padded_segments_that_are_really_padded(lcgs, oracle):
    """three steps without read-back: in steps 2 and 3 every message holds padded(n) > n rows, the 2-D rows of view v sit at
    gin_off[v] = v * count, positions beyond the true counts are addressed and must stay out of the result.  The byte counts
    say that steps 2 and 3 ran without read-back: each message is padded(n) rows of (4 + 48) bytes out and 48 back."""
    views = padding_premise(oracle)
    steps = [views] * 3
    out = _steps(views[0].scene, 3, steps, True)
    _check_all(out, steps, "B3 padded", True)
    # the table of the step as the kernels count it (between hit and on): one projection per (owner, view)
    r = _renderer(views[0].scene)
    t = [[int(r.owner_project(0, v.cam(), f, c)[0].shape[0]) for v in views] for f, c in _ranges(12000, 3)]
    for me, (snaps, _) in enumerate(out):
        others = [o for o in range(3) if o != me]
        exact = sum(t[me][o] * 52 + t[o][me] * 48 for o in others) + 24
        padded = sum(_padded(t[me][o], 4000) * 52 + _padded(t[o][me], 4000) * 48 for o in others) + 24
        assert padded > exact
        assert [s["stats"]["bytes_sent"] for s in snaps] == [exact, padded, padded], (me, [s["stats"] for s in snaps], exact, padded)
        assert [s["redo"] for s in snaps] == [0, 0, 0]
        assert all(s["stats"]["touched_rows"] == sum(t[o][me] for o in range(3)) for s in snaps)


def clipped_premise(oracle):
    """the scene and poses of test_gpu_owner's clipped-step test at P = 9001: step 1 looks away (every (owner, view) count
    small), step 2 at the scene -- some (owner, view) holds more rows than a message sized by step 1's count"""
    def make():
        scene = make_scene(np.random.default_rng(91), 9001, log_scale=(-4.0, 0.8))
        angles = np.linspace(0.0, 1.0, 3)
        at = [View(oracle, scene, ([-3 * np.cos(a), -0.5 + 3 * np.sin(a), 2.3], [0, 0, 0.5], [0, 0, 1]), W, H, seed=50 + i)
              for i, a in enumerate(angles)]
        away = [View(oracle, scene, ([-3 * np.cos(a), -0.5 + 3 * np.sin(a), 2.3], [-9 * np.cos(a), 6 * np.sin(a), 8.0], [0, 0, 1]),
                     W, H, seed=60 + i) for i, a in enumerate(angles)]
        return away, at
    away, at = cached("own B4", make)
    t_away, t_hit = _table(away), _table(at, [v.hit for v in at])
    counts = [c for _, c in _ranges(9001, 3)]
    assert any(t_hit[o][v] > _padded(t_away[o][v], counts[o]) for o in range(3) for v in range(3)), (t_away, t_hit)
    return away, at


def test_a_clipped_step_is_repeated(lcgs, oracle):
    """redos == [0, 1, 0]; the gradients are held per row after the repeated step and after the third (the first step looks
    away: its frame is not the subject)"""
    away, at = clipped_premise(oracle)
    steps = [away, at, at]
    out = _steps(at[0].scene, 3, steps, True)
    for me, (snaps, _) in enumerate(out):
        assert [s["redo"] for s in snaps] == [0, 1, 0], (me, [s["redo"] for s in snaps])
        for s in (1, 2):
            _check_step(snaps[s], at, me, f"B4 clipped rank {me} step {s}", False, True)
