"""`-m gpu`: every dispatch path of the dense / compact / fused backward held to the per-row bound
(gpu_util.check_gradient_rows, unchanged) -- the routes beside the one test_gpu_backward.py and test_gpu_gradient_rows.py take:

  A  per-stage profiling (in-order forward, memset fill, launch_zero_grads2d, no persistent grid), the hand-over between the
     pipelined and the in-order frame, the mode switched between a frame and its backward, a second and third backward of one frame;
  B  the preprocess-backward run as splat-range slices (LCGS_GRAD_SLICES through a world-size-1 communicator): empty slices,
     one-row slices, 2 / 4 / 16 slices, P either side of the 4096 rule, accumulate and profiling under slices;
  C  a backward whose grid is smaller than the on-screen count (the launch hint of an earlier, nearly empty frame): the
     grid-stride loops of the three per-splat kernels take several passes;
  D  on-screen counts V at wave and block boundaries, dense and compact, in each of the per-splat kernels;
  E  fit_views (the bounded persistent render-backward beside the next view's forward) and the LOD cull, per row.

Every gradient array starts at 7.0, every case first asserts on the oracle that the frame is what it claims to be (the
`*_premise` functions need no GPU), and each (scene, pose, dL/dimg) computes its oracle frame and its bound once (_View)."""
import numpy as np
import pytest
import torch

import luisacomputegaussiansplatting_amd as L
from conftest import make_scene
from gpu_util import BG, DEV, KEYS, View as _View, assert_image_parity, cached as _cached, check_gradient_rows, dev
from gpu_util import sevens as _sevens, sum_bounds as _sum_bounds

pytestmark = pytest.mark.gpu
POSE = ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1])
POSE2 = ([2.5, 1.5, 1.0], [0, 0, 0.5], [0, 0, 1])
LR = {"pos": 1.6e-4, "sh_dc": 2.5e-3, "sh_rest": 1.25e-4, "opacity": 5e-2, "scale": 5e-3, "rot": 1e-3}
def _renderer(scene, sh_deg=3, ctx=None):
    r = L.Renderer(ctx or L.Context(0))
    d = {k: dev(scene[k]) for k in KEYS}
    r.bind_scene(*[d[k] for k in KEYS], sh_degree=sh_deg)
    return r, d


def _forward(r, view, sync=True):
    img = torch.zeros(3, view.H, view.W, device=DEV)
    n = r.forward(view.cam(), img, bg=view.bg, keep_state=True, sync=sync)
    assert n is None or n == view.ref["num_rendered"], (n, view.ref["num_rendered"])
    return img


def _run(r, view, tag, sync=True, g=None, between=None, bound=None, check_image=True, **backward_kw):
    """forward (keep_state) -> backward onto 7.0-filled arrays (or onto g) -> the frame bit-identical to the oracle's, every
    row of every attribute within its bound; returns (the oracle's render, the gradient arrays)"""
    img = _forward(r, view, sync)
    if between is not None:
        between()
    g = g if g is not None else _sevens(view.scene)
    r.backward(dev(view.dL), *[g[k] for k in KEYS], **backward_kw)
    r.ctx.synchronize()  # (an asynchronous frame's image is read only now)
    if check_image:
        assert_image_parity(img.cpu().numpy(), view.ref)
    view.survivors(r)
    check_gradient_rows(g, None, None, None, bound=bound if bound is not None else view.bound(), tag=tag)
    return view.ref, g


def _off_screen_block(scene, lo, hi):
    scene["pos"][lo:hi] += 100.0
    return scene


# ------------------------------------------------------------------------------------------ A: profiling and its transitions
def profiling_premise(oracle):
    """20 000 splats, rows [8000, 12000) moved off screen, 320 x 240, two poses, two dL/dimg for the first pose"""
    def make():
        scene = _off_screen_block(make_scene(np.random.default_rng(101), 20000), 8000, 12000)
        v0, v1 = _View(oracle, scene, POSE, 320, 240, seed=0), _View(oracle, scene, POSE2, 320, 240, seed=1)
        for v in (v0, v1):
            assert not v.on[8000:12000].any() and v.V >= 8000, v.V
        assert not np.array_equal(v0.ref["img"], v1.ref["img"])
        return v0, v1, v0.other_dL(2)
    return _cached("A", make)


def _stage_times_ok(t):
    assert t and all(np.isfinite(ms) and ms >= 0 for ms in t.values()), t


def test_frame_under_profiling(lcgs, oracle):
    """lcgs_set_profiling(1): the in-order forward, the five memsets ("zero_grads"), launch_zero_grads2d, the plain
    render-backward grid -- the mode every per-stage figure is measured in renders the oracle's frame and its gradients"""
    v0, _, _ = profiling_premise(oracle)
    r, _ = _renderer(v0.scene)
    r.set_profiling(True)
    img = _forward(r, v0)
    assert_image_parity(img.cpu().numpy(), v0.ref)
    fwd = r.stage_times()
    _stage_times_ok(fwd)
    assert "render" in fwd
    g = _sevens(v0.scene)
    r.backward(dev(v0.dL), *[g[k] for k in KEYS])
    bwd = r.stage_times()
    r.ctx.synchronize()
    _stage_times_ok(bwd)
    names = [n for n in bwd if n in ("zero_grads", "render_backward", "preprocess_backward")]
    assert names == ["zero_grads", "render_backward", "preprocess_backward"], list(bwd)
    check_gradient_rows(g, None, None, None, bound=v0.bound(), tag="profiling on")
    r.set_profiling(False)
    _forward(r, v0)
    assert r.stage_times() == {}


@pytest.mark.parametrize("sync", [True, False], ids=["sync", "async"])
def test_profiling_switched_between_frames(lcgs, oracle, sync):
    """off -> on -> on -> off -> off on one context, two poses alternating: the hand-over from pipelined to in-order frames
    (the auxiliary stream's pending fill and tile schedule; only asynchronous frames leave any pending) and the way back (every
    zeroed workspace copy marked stale).  An asynchronous frame's image is read after the context is synchronised."""
    v0, v1, _ = profiling_premise(oracle)
    r, _ = _renderer(v0.scene)
    for i, on in enumerate([False, True, True, False, False]):
        r.set_profiling(on)
        _run(r, (v0, v1)[i % 2], f"frame {i} profiling {'on' if on else 'off'} {'sync' if sync else 'async'}", sync=sync)


@pytest.mark.parametrize("first", [False, True], ids=["off_then_on", "on_then_off"])
def test_profiling_switched_between_a_frame_and_its_backward(lcgs, oracle, first):
    """g2d_zeroed set by a frame rendered in one mode, consumed by a backward in the other"""
    v0, v1, _ = profiling_premise(oracle)
    r, _ = _renderer(v0.scene)
    r.set_profiling(first)
    _run(r, v0, f"forward {'on' if first else 'off'}, backward {'off' if first else 'on'}",
         between=lambda: r.set_profiling(not first))
    _run(r, v1, "the next frame in the backward's mode")


def test_second_and_third_backward_of_one_frame(lcgs, oracle):
    """the first backward consumes the renderer's cleared 2-D rows; the second (another dL/dimg) must clear them itself; a
    third with accumulate adds the first's gradients onto the second's: the sum of the two bounds and f64 references"""
    v0, _, v0b = profiling_premise(oracle)
    r, _ = _renderer(v0.scene)
    _, g = _run(r, v0, "first backward")
    g = _sevens(v0.scene)
    r.backward(dev(v0b.dL), *[g[k] for k in KEYS])
    r.ctx.synchronize()
    check_gradient_rows(g, None, None, None, bound=v0b.bound(), tag="second backward")
    r.backward(dev(v0.dL), *[g[k] for k in KEYS], accumulate=True)
    r.ctx.synchronize()
    check_gradient_rows(g, None, None, None, bound=_sum_bounds([v0, v0b]), tag="third backward, accumulated")


def low_degree_premise(oracle, deg):
    def make():
        scene = _off_screen_block(make_scene(np.random.default_rng(110 + deg), 5000), 2000, 3000)
        scene["sh"] = np.ascontiguousarray(scene["sh"][:, :(deg + 1) ** 2 * 3])
        v = _View(oracle, scene, POSE, 160, 120, seed=3, sh_deg=deg)
        assert not v.on[2000:3000].any() and v.V >= 2000, v.V
        return v
    return _cached(("A5", deg), make)


@pytest.mark.parametrize("deg", [0, 1])
def test_low_sh_degrees_under_profiling(lcgs, oracle, deg):
    """the memset of dL_dsh is P * (deg + 1)^2 * 3 floats long"""
    v = low_degree_premise(oracle, deg)
    r, _ = _renderer(v.scene, sh_deg=deg)
    r.set_profiling(True)
    _run(r, v, f"degree {deg}, profiling on")


# ------------------------------------------------------------------------------------------ B: the sliced preprocess-backward
SLICE_SCENES = ("P4096", "P4097", "first_half_off", "last_quarter_off", "two_rows", "all_off")


def slice_counts(on, P, K):
    """survivors per splat range [k P / K, (k + 1) P / K), the integer arithmetic of k_slice_bounds"""
    idx = np.nonzero(on)[0]
    edges = [(P * k) // K for k in range(K + 1)]
    return [int(((idx >= edges[k]) & (idx < edges[k + 1])).sum()) for k in range(K)]


def sliced_premise(oracle, name, K):
    """the scene `name` at 200 x 150 with the survivor counts per slice it claims for K slices asserted"""
    def make():
        P = {"P4096": 4096, "P4097": 4097, "P4095": 4095}.get(name, 8192)
        scene = make_scene(np.random.default_rng(200 + P + len(name)), P, spread=0.3)
        if name.startswith("P40") or name == "last_quarter_off":  # row 0 survives: the first boundary is the one whose error
            scene["pos"][0], scene["scale"][0], scene["opacity"][0] = [-1.5, -0.25, 1.4], 0.02, 0.6  # loses a row (in front of the cloud)
        if name.startswith("P40"):
            scene["pos"][100:137] += 100.0  # (4096 survivors would split into multiples of 64)
        elif name == "first_half_off":
            scene["pos"][:P // 2] += 100.0
        elif name == "last_quarter_off":
            scene["pos"][P - P // 4:] += 100.0
        elif name in ("two_rows", "all_off"):
            keep = [P // K + 5, P - 3] if name == "two_rows" else []
            for i in keep:  # on the target, a few pixels wide
                scene["pos"][i] = np.array(POSE[1], np.float32) + np.float32(0.05) * np.float32(i == keep[0])
                scene["scale"][i], scene["opacity"][i] = 0.03, 0.6
            off = np.ones(P, bool)
            off[keep] = False
            scene["pos"][off] += 100.0
        return _View(oracle, scene, POSE, 200, 150, seed=4)
    # (two_rows places its first row by K; every other scene serves all K)
    v = _cached(("B", name, K if name == "two_rows" else 0), make)
    for rows in (v.on, v.hit):  # the frame's survivors lie between the two
        slice_claim(name, rows, v.P, K)
    return v


def slice_claim(name, on, P, K):
    """what the scene `name` claims about the survivors per slice, asserted on the row mask `on`"""
    c = slice_counts(on, P, K)
    assert sum(c) == on.sum()
    if name in ("P4096", "P4097", "P4095"):
        assert min(c) > 0 and any(n % 64 for n in c) and on[0], c
    elif name == "first_half_off":
        assert not any(c[:K // 2]) and min(c[K // 2:]) > 0, c
    elif name == "last_quarter_off":
        empty = [k for k in range(K) if (P * k) // K >= P - P // 4]  # (none of 2 slices: the last one is half empty)
        assert len(empty) == K // 4 and not any(c[k] for k in empty) and all(c[k] for k in range(K) if k not in empty), c
        assert not on[P - P // 4:].any() and on[0]
    elif name == "two_rows":
        want = [0] * K
        want[1] += 1
        want[-1] += 1  # (2 slices: slice 1 is the last one and holds both)
        assert c == want, c
    elif name == "all_off":
        assert not on.any()


def _comm_renderer(monkeypatch, view, K):
    """a context bound to the view's scene with a world-size-1 communicator that asks for K gradient slices (read from the
    environment when the communicator is created)"""
    monkeypatch.setenv("LCGS_GRAD_SLICES", str(K))
    r, d = _renderer(view.scene)
    return r, L.Comm(r.ctx, 0, 1)


@pytest.mark.parametrize("K", [2, 4, 16])
@pytest.mark.parametrize("name", SLICE_SCENES)
def test_sliced_backward(lcgs, oracle, monkeypatch, name, K):
    v = sliced_premise(oracle, name, K)
    r, comm = _comm_renderer(monkeypatch, v, K)
    try:
        if v.V == 0:  # an empty frame: the forward leaves the image alone, the backward zero-fills and succeeds
            img = torch.zeros(3, v.H, v.W, device=DEV)
            assert r.forward(v.cam(), img, bg=v.bg, keep_state=True) == 0
            g = _sevens(v.scene)
            r.backward(dev(v.dL), *[g[k] for k in KEYS])
            r.ctx.synchronize()
            assert all(not g[k].any() for k in KEYS)
            check_gradient_rows(g, None, None, None, bound=v.bound(), tag=f"{name} / {K} slices")
        else:
            _run(r, v, f"{name} / {K} slices")
        got = np.zeros(v.P, bool)
        got[v.survivors(r)] = True
        slice_claim(name, got, v.P, K)
    finally:
        comm.close()


def test_sliced_backward_below_the_4096_rule_runs_unsliced(lcgs, oracle, monkeypatch):
    v = sliced_premise(oracle, "P4095", 16)
    r, comm = _comm_renderer(monkeypatch, v, 16)
    try:
        _run(r, v, "P = 4095, 16 slices asked for")
    finally:
        comm.close()


def test_sliced_backward_accumulates_two_views(lcgs, oracle, monkeypatch):
    v0 = sliced_premise(oracle, "last_quarter_off", 4)
    v1 = _cached("B accumulate", lambda: _View(oracle, v0.scene, POSE2, 200, 150, seed=5))
    assert v1.V > 0 and min(slice_counts(v1.on, v1.P, 4)[:3]) > 0
    r, comm = _comm_renderer(monkeypatch, v0, 4)
    try:
        _, g = _run(r, v0, "4 slices, first view")
        _run(r, v1, "4 slices, two views accumulated", g=g, accumulate=True, bound=_sum_bounds([v0, v1]))
    finally:
        comm.close()


def test_sliced_backward_under_profiling_and_the_allreduce_of_one(lcgs, oracle, monkeypatch):
    """profiling on: the fill and k_slice_bounds share the main stream.  Then the one all-reduce of this file: a world of one
    sums to itself, so the arrays are unchanged."""
    v = sliced_premise(oracle, "first_half_off", 4)
    r, comm = _comm_renderer(monkeypatch, v, 4)
    try:
        r.set_profiling(True)
        _run(r, v, "4 slices, profiling on")
        r.set_profiling(False)
        _, g = _run(r, v, "4 slices, profiling off again")
        before = {k: g[k].clone() for k in KEYS}
        comm.allreduce_grads(g)
        r.ctx.synchronize()
        torch.cuda.synchronize()
        assert all(torch.equal(g[k], before[k]) for k in KEYS)
    finally:
        comm.close()


# ------------------------------------------------------------------------------------------ C: a grid smaller than V
FEW_POSE = ([47.0, 49.5, 2.3], [50.0, 50.0, 0.5], [0, 0, 1])  # looks at the far cluster, the cloud behind it


def strided_premise(oracle):
    """30 000 splats at 400 x 300: 150 of them in a cluster far away.  FEW_POSE sees only (some of) the cluster, POSE the cloud."""
    def make():
        rng = np.random.default_rng(300)
        scene = make_scene(rng, 30000)
        scene["pos"][::200] = (rng.normal(0, 0.3, (150, 3)) + np.array(FEW_POSE[1])).astype(np.float32)
        few, many = _View(oracle, scene, FEW_POSE, 400, 300, seed=6), _View(oracle, scene, POSE, 400, 300, seed=7)
        assert few.hit.any() and few.V <= 200 and many.hit.sum() >= 15000, (int(few.hit.sum()), few.V, int(many.hit.sum()))
        # the hint the synchronous frame leaves (abi_frame.cpp: V + V / 4 + 4096), as blocks of 256 rows
        blocks = (few.V + few.V // 4 + 4096 + 255) // 256
        assert many.hit.sum() > 3 * 256 * blocks, blocks  # the unsliced loops take at least 4 passes
        return few, many
    return _cached("C", make)


def _under_hinted_frame(r, few, many):
    """A synchronous frame with a handful of survivors sets the context's launch hint to V + V / 4 + 4096 (lcgs_render_forward,
    the lines after `launch-size hints for the following asynchronous frames`); an asynchronous frame returns before those
    lines (`fully asynchronous frame`), so the hint stays at most 4346 while >= 15 000 splats reach the screen.  The backward
    sizes its per-splat launch grid_256(hint) (grid_256(hint / slices) per slice): `blk += gridDim.x` runs >= 4 times, with the
    block-wide barriers inside the loop.  No accessor shows the hint: the premise rests on reading those lines."""
    img = torch.zeros(3, few.H, few.W, device=DEV)
    assert r.forward(few.cam(), img, bg=few.bg, sync=True) == few.ref["num_rendered"]
    return _forward(r, many, sync=False)


@pytest.mark.parametrize("path", ["dense", "16_slices", "compact"])
def test_strided_backward_behind_an_under_hinted_frame(lcgs, oracle, monkeypatch, path):
    few, many = strided_premise(oracle)
    comm = None
    if path == "16_slices":
        blocks = ((few.V + few.V // 4 + 4096) // 16 + 255) // 256  # grid_256(hint / slices)
        assert min(slice_counts(many.hit, many.P, 16)) > 256 * blocks  # every slice takes more than one pass
        r, comm = _comm_renderer(monkeypatch, many, 16)
    else:
        r, _ = _renderer(many.scene)
    try:
        img = _under_hinted_frame(r, few, many)
        g = _sevens(many.scene)
        r.backward(dev(many.dL), *[g[k] for k in KEYS], compact=path == "compact")
        r.ctx.synchronize()
        assert_image_parity(img.cpu().numpy(), many.ref)
        if path == "compact":
            rows = many.survivors(r)
            check_gradient_rows({k: g[k].reshape(many.P, -1)[:rows.size] for k in KEYS}, None, None, None, bound=many.bound(),
                                rows=rows, tag="under-hinted, compact")
            assert all((g[k].reshape(many.P, -1)[rows.size:] == 7.0).all() for k in KEYS)  # nothing written past row V
        else:
            many.survivors(r)
            check_gradient_rows(g, None, None, None, bound=many.bound(), tag=f"under-hinted, {path}")
    finally:
        if comm is not None:
            comm.close()


def _activate(raw):
    return {"pos": raw["pos"], "scale": torch.exp(raw["scale"]), "sh": raw["sh"], "opacity": torch.sigmoid(raw["opacity"]),
            "rotq": raw["rotq"] / raw["rotq"].norm(dim=1, keepdim=True)}


def test_strided_fused_adam_behind_an_under_hinted_frame(lcgs, oracle):
    """lcgs_render_backward_adam with a grid of <= 17 blocks for >= 15 000 on-screen splats, against backward(compact) +
    adam_step(visible_only, compact_grads) on a twin context with a full-size grid: the bars of
    test_gpu_train.py::test_backward_with_the_optimiser_folded_in_equals_the_two_calls (two backward passes of one frame differ
    in the last bits of their float atomics; Adam's first step turns the sign of a near-zero gradient into +-lr)"""
    few, many = strided_premise(oracle)
    sc = many.scene
    raw0 = {"pos": sc["pos"], "scale": np.log(sc["scale"]), "rotq": sc["rotq"] * 1.3, "sh": sc["sh"],
            "opacity": np.log(sc["opacity"] / (1 - sc["opacity"]))}
    raw0 = {k: dev(np.asarray(a, np.float32)) for k, a in raw0.items()}
    lr_of = {"pos": LR["pos"], "scale": LR["scale"], "rotq": LR["rot"], "sh": LR["sh_dc"], "opacity": LR["opacity"]}
    out = {}
    for fused in (False, True):
        raw = {k: t.clone() for k, t in raw0.items()}
        act = {k: t.clone() for k, t in _activate(raw).items()}
        act["pos"], act["sh"] = raw["pos"], raw["sh"]
        m, v = ({k: torch.zeros_like(raw[k]) for k in KEYS} for _ in range(2))
        r = L.Renderer(L.Context(0))
        r.bind_scene(*[act[k] for k in KEYS])
        if fused:
            _under_hinted_frame(r, few, many)
            r.backward_adam(dev(many.dL), raw, m, v, act, 1, LR, eps=1e-8)
        else:
            _forward(r, many, sync=False)
            g = {k: torch.zeros_like(raw[k]) for k in KEYS}
            r.backward(dev(many.dL), *[g[k] for k in KEYS], compact=True)
            r.adam_step(g, raw, m, v, act, 1, LR, eps=1e-8, visible_only=True, compact_grads=True)
        r.ctx.synchronize()
        out[fused] = (raw, torch.from_numpy(many.survivors(r)).to(DEV).long())
    (raw_a, rows), (raw_b, rows_b) = out[False], out[True]
    assert torch.equal(rows, rows_b)
    off = torch.ones(many.P, dtype=torch.bool, device=DEV)
    off[rows] = False
    # the rows that took a step (any element of any attribute moved; a row whose gradients are all 0 does not move) are the
    # twin's: no pass of the loop skipped
    moved = [sum((raw[k] != raw0[k]).reshape(many.P, -1).any(dim=1) for k in KEYS) > 0 for raw in (raw_a, raw_b)]
    assert torch.equal(moved[0], moved[1]) and moved[0].any(), (int(moved[0].sum()), int(moved[1].sum()))
    for k in KEYS:
        assert not torch.equal(raw_b[k][rows], raw0[k][rows]), k  # it trained ...
        assert torch.equal(raw_b[k][off], raw0[k][off]), k  # ... and only the on-screen rows
        diff = (raw_b[k] - raw_a[k]).abs()
        assert float(diff.max()) <= 2.02 * lr_of[k], (k, float(diff.max()))
        assert float((diff > 0.05 * lr_of[k]).float().mean()) < 0.01, k


# ------------------------------------------------------------------------------------------ D: V at wave / block boundaries
BOUNDARY_V = (1, 63, 64, 65, 255, 256, 257, 513)


def boundary_premise(oracle, V, deg=3):
    """P = 1000 at 96 x 80 with exactly V rows on screen: whether a row reaches the screen depends on that row alone, so V of
    the rows the full scene shows are kept (spread over the index range) and every other row moves off screen"""
    def make():
        rng = np.random.default_rng(400)
        scene = make_scene(rng, 1000, spread=0.25, log_scale=(-3.5, 0.7))
        scene["sh"] = np.ascontiguousarray(scene["sh"][:, :(deg + 1) ** 2 * 3])
        shown = np.nonzero(_View(oracle, dict(scene), POSE, 96, 80, seed=8, sh_deg=deg).hit)[0]  # (with the others gone
        assert shown.size >= V, shown.size  # a row is hidden by fewer rows: it still reaches its pixels)
        keep = np.sort(rng.choice(shown, V, replace=False))
        off = np.ones(1000, bool)
        off[keep] = False
        scene["pos"][off] += 100.0
        v = _View(oracle, scene, POSE, 96, 80, seed=8, sh_deg=deg)
        assert v.V == V and np.array_equal(np.nonzero(v.on)[0], keep) and np.array_equal(v.hit, v.on)  # exactly V survive
        return v
    return _cached(("D", V, deg), make)


def _dense_and_compact(r, v, tag, sh_offset=0):
    """one frame, its dense backward, then its compact backward (rows mapped through visible_rows)"""
    _run(r, v, f"{tag} dense", g=_sevens(v.scene, sh_offset))
    rows = v.survivors(r)
    assert rows.size == v.V
    g = _sevens(v.scene, sh_offset)
    r.backward(dev(v.dL), *[g[k] for k in KEYS], compact=True)
    r.ctx.synchronize()
    check_gradient_rows({k: g[k].reshape(v.P, -1)[:v.V] for k in KEYS}, None, None, None, bound=v.bound(), rows=rows,
                        tag=f"{tag} compact")
    assert all((g[k].reshape(v.P, -1)[v.V:] == 7.0).all() for k in KEYS)  # nothing written past row V


@pytest.mark.parametrize("V", BOUNDARY_V)
def test_on_screen_counts_at_wave_and_block_boundaries(lcgs, oracle, V):
    """degree 3, 16-byte-aligned dL_dsh: the kernel that works from the kept colour Jacobian, whose waves write the SH rows
    cooperatively (`slot < nvalid` matters in a partly filled wave only)"""
    v = boundary_premise(oracle, V)
    r, _ = _renderer(v.scene)
    _dense_and_compact(r, v, f"V={V}")


@pytest.mark.parametrize("V", [65, 257])
def test_boundary_counts_with_an_unaligned_sh_gradient(lcgs, oracle, V):
    """dL_dsh one float past a 16-byte boundary: k_preprocess_backward, lane-wise SH rows"""
    v = boundary_premise(oracle, V)
    r, _ = _renderer(v.scene)
    _dense_and_compact(r, v, f"V={V} unaligned dL_dsh", sh_offset=1)


@pytest.mark.parametrize("V", [65, 257])
def test_boundary_counts_at_degree_2(lcgs, oracle, V):
    v = boundary_premise(oracle, V, deg=2)
    r, _ = _renderer(v.scene, sh_deg=2)
    _dense_and_compact(r, v, f"V={V} degree 2")


# ------------------------------------------------------------------------------------------ E: fit_views and the LOD cull
def fit_views_premise(oracle):
    """the scene recipe and the three poses of test_gpu_train.py's fit-views test (30 000 splats here: the per-row checker's
    size limit), targets = the oracle's frames of a perturbed scene.  With LOSS_PHOTOMETRIC and lambda = 0 the gradient image
    of a view is float(sign(img - target) / n) bit for bit, and img is the oracle's frame bit for bit (asserted on the GPU)."""
    def make():
        from bench import view_pose

        rng = np.random.default_rng(77)
        P, W, H = 30000, 320, 240
        scene = make_scene(rng, P, spread=1.5, log_scale=(-3.6, 0.6))
        moved = dict(scene)
        moved["pos"] = scene["pos"] + rng.normal(0, 0.01, (P, 3)).astype(np.float32)
        moved["sh"] = scene["sh"] + rng.normal(0, 0.05, (P, 48)).astype(np.float32)
        views, targets = [], []
        for k in range(3):
            ocam = oracle.lookat(*view_pose(k), width=W, height=H)
            ref, target = oracle.render(scene, ocam, bg=BG), oracle.render(moved, ocam, bg=BG)["img"]
            sgn = (ref["img"] > target).astype(np.float64) - (ref["img"] < target)
            assert (sgn != 0).mean() > 0.5
            views.append(_View(oracle, scene, view_pose(k), W, H, bg=BG, dL=(sgn / (3 * W * H)).astype(np.float32), ref=ref))
            targets.append(target)
            assert views[-1].V >= 1000, views[-1].V
        return views, targets
    return _cached("E fit", make)


def test_fit_views_per_row(lcgs, oracle):
    """lcgs_fit_views: three views alternating between the context and its sibling, the render-backward on its bounded
    persistent grid beside the next view's forward, the dense rows summed over the views -- held to the sum of the three
    views' bounds against the sum of their f64 references; two steps on one context"""
    views, targets = fit_views_premise(oracle)
    r, _ = _renderer(views[0].scene)
    for v in views:  # the frames fit_views forms its loss gradients from
        img = torch.zeros(3, v.H, v.W, device=DEV)
        assert r.forward(v.cam(), img, bg=v.bg) == v.ref["num_rendered"]
        assert_image_parity(img.cpu().numpy(), v.ref)
    r.set_fit_loss(L.LOSS_PHOTOMETRIC, 0.0)
    t = [dev(x) for x in targets]
    bound = _sum_bounds(views)
    for step in range(2):
        g = _sevens(views[0].scene)
        losses = torch.full((3,), -1.0, device=DEV)
        torch.cuda.synchronize()
        r.fit_views([v.cam() for v in views], t, *[g[k] for k in KEYS], losses, bg=BG)
        r.ctx.synchronize()
        assert (losses > 0).all() and torch.isfinite(losses).all()
        check_gradient_rows(g, None, None, None, bound=bound, tag=f"fit_views, step {step}")


def lod_premise(oracle, min_radius=4):
    """20 000 splats at 320 x 240, many a pixel wide: the rule (radius < min_radius px -> dropped) takes 10 % .. 50 % of the
    on-screen splats.  The frame is the oracle's frame of the scene WITHOUT those rows (order kept, so equal depths blend as
    before); the kept rows' gradients are that sub-scene's."""
    def make():
        scene = make_scene(np.random.default_rng(31), 20000, log_scale=(-4.6, 0.8))
        full = _View(oracle, scene, POSE, 320, 240, seed=9)
        dropped = (full.ref["radii"] > 0) & (full.ref["radii"] < min_radius)
        share = (dropped & full.on).sum() / full.V
        assert 0.10 <= share <= 0.50, share
        keep = ~dropped
        sub = _View(oracle, {k: np.ascontiguousarray(scene[k][keep]) for k in KEYS}, POSE, 320, 240, dL=full.dL)
        oracle.set_lod_min_radius(min_radius)
        try:
            ruled = oracle.render(scene, full.ocam, bg=BG)
        finally:
            oracle.set_lod_min_radius(0)
        # row removal IS the rule: the same frame bit for bit, the same radii on the kept rows
        assert np.array_equal(ruled["img"].view(np.uint32), sub.ref["img"].view(np.uint32))
        assert ruled["num_rendered"] == sub.ref["num_rendered"] and np.array_equal(ruled["radii"][keep], sub.ref["radii"])
        return full, sub, keep
    return _cached("E lod", make)


def test_lod_cull_per_row(lcgs, oracle):
    full, sub, keep = lod_premise(oracle)
    r, _ = _renderer(full.scene)
    r.set_lod(4)
    img = torch.zeros(3, full.H, full.W, device=DEV)
    assert r.forward(full.cam(), img, bg=BG, keep_state=True) == sub.ref["num_rendered"]
    assert_image_parity(img.cpu().numpy(), sub.ref)
    g = _sevens(full.scene)
    r.backward(dev(full.dL), *[g[k] for k in KEYS])
    r.ctx.synchronize()
    gone = torch.from_numpy(np.nonzero(~keep)[0]).to(DEV)
    assert all(not g[k][gone].any() for k in KEYS)  # dropped rows: exactly 0
    kept = torch.from_numpy(np.nonzero(keep)[0]).to(DEV)
    check_gradient_rows({k: g[k][kept] for k in KEYS}, None, None, None, bound=sub.bound(), tag="LOD, kept rows")
