"""`-m gpu`: a chained frame's cull pass one slot ahead.  A pipelined frame that chains behind another runs
k_cull_compact on the context's cull stream, beside the previous head's sort chain: it waits for that head's first scatter and
for nothing else, and its own head joins it in front of k_rowscan_first.  Every cull pass must still see its own camera and
the scene of its place in the stream, and the slabs, chunk counts and first digit counts of one frame must not leak into the
next.  As in test_gpu_pipelined_frames.py every comparison is bit equality (torch.equal) with the same frame rendered alone by
a synchronising call on a fresh context; the helpers are copied from that file, and the references share its cache entries.

A chained frame culls early only while the GPU is behind the host (one event query per frame, the one that gates the bounded
renderer grid), so every burst whose count is asserted is queued behind a long matrix product on the caller's stream: then
each frame finds its predecessor's renderer unfinished, and exactly the chained frames cull early.  One burst runs without it:
there the count depends on host timing and only its bounds are asserted, beside the images.

The whole file runs again in child processes under LCGS_EARLY_CULL=0 (chained frames cull on the head stream: the counter
stays 0, the images are the same) and under LCGS_PIPELINE=0 (single-stream order)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, make_scene
from gpu_util import DEV, KEYS, cached, check_gradient_rows, dev, gradient_row_bound

pytestmark = pytest.mark.gpu

BG = (0.1, 0.2, 0.3)
P_SCENE = 20000  # ten 2048-splat cull chunks, the last one partial
P_SMALL = 5000   # three chunks: another row stride of the digit-count table, shorter slabs
POSES = [([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1]), ([2.5, -2.0, 1.2], [0, 0, 0.5], [0, 0, 1]),
         ([0.3, 3.2, 0.9], [0, 0, 0.5], [0, 0, 1]), ([-1.5, -2.8, 3.0], [0.2, 0.1, 0.4], [0, 0, 1])]
AWAY = ([-3, -0.5, 2.3], [-6, -1.0, 4.1], [0, 0, 1])
SIZES = [(256, 144), (250, 130)]
# a camera twice in a row (1 1, 3 3), the view that renders nothing (4) between two that do, and twice in a row itself
HELD_ORDER = [0, 1, 1, 4, 2, 3, 3, 4, 4, 0, 2, 1]

PIPELINE_ON = os.environ.get("LCGS_PIPELINE") != "0"
EARLY_ON = PIPELINE_ON and os.environ.get("LCGS_EARLY_CULL") != "0"


def _scene(seed=5):
    return cached(("pipelined scene", seed), lambda: make_scene(np.random.default_rng(seed), P_SCENE))


def _small_scene():
    return cached("early cull small scene", lambda: make_scene(np.random.default_rng(8), P_SMALL))


def _cams(lcgs, W, H, poses=POSES + [AWAY]):
    return [lcgs.get_lookat_cam(*p, width=W, height=H) for p in poses]


def _owned(lcgs, scene, policy=None):
    r = lcgs.Renderer(lcgs.Context(0))
    r.upload_scene(scene)
    if policy:
        r.set_list_policy(policy)
    return r


def _alone(lcgs, r, cam, W, H):
    """one frame by a synchronising call: (image, num_rendered); the image starts at -1 (an untouched one stays there)"""
    img = torch.full((3, H, W), -1.0, device=DEV)
    n = r.forward(cam, img, bg=BG, sync=True)
    return img, n


def _refs(lcgs, W, H, policy=None, seed=5):
    """the four views (and the view turned away) of the scene, each rendered alone on a fresh context: computed once"""
    def make():
        r = _owned(lcgs, _scene(seed), policy)
        out = [_alone(lcgs, r, c, W, H) for c in _cams(lcgs, W, H)]
        assert all(n > 0 for _, n in out[:4]) and out[4][1] == 0 and bool((out[4][0] == -1.0).all())
        assert not any(torch.equal(out[i][0], out[j][0]) for i in range(4) for j in range(i))  # four different images
        return [img for img, _ in out]
    return cached(("pipelined refs", W, H, policy, seed), make)


def _small_refs(lcgs, W, H):
    def make():
        r = _owned(lcgs, _small_scene())
        out = [_alone(lcgs, r, c, W, H) for c in _cams(lcgs, W, H)]
        assert all(n > 0 for _, n in out[:4]) and out[4][1] == 0
        return [img for img, _ in out]
    return cached(("early cull small refs", W, H), make)


def _enqueue(r, cams, imgs, order):
    """frames order[k] -> imgs[k % len(imgs)] without read-back; the image is cloned on the stream behind each call.  Every
    image is refilled with -1 in front of its frame (on the stream), so the view that renders nothing leaves -1 behind"""
    out = []
    for k, c in enumerate(order):
        img = imgs[k % len(imgs)]
        img.fill_(-1.0)
        r.forward(cams[c], img, bg=BG, sync=False)
        out.append(img.clone())
    return out


def _counts(r):
    return dict(r.pipeline_counts(), early=r.early_cull_count())


def _assert_counts(r, frames, chained, held=True):
    """what the context itself says it did since its held-back bursts began (_held_burst notes the counts in front of the
    first one): without this a library that never culled early would pass every comparison.
    held: the bursts were queued behind _hold_back(), so every chained frame found the GPU behind the host"""
    base = getattr(r, "_early_cull_base", {"piped": 0, "chained": 0, "bounded": 0, "early": 0})
    now = _counts(r)
    d = {k: now[k] - base[k] for k in now}
    if PIPELINE_ON:
        assert d["piped"] == frames and d["chained"] == chained, (d, base)
    else:
        assert now == {"piped": 0, "chained": 0, "bounded": 0, "early": 0}, now
    if held:
        assert d["early"] == (chained if EARLY_ON else 0), (d, base)
    else:
        assert 0 <= d["early"] <= (chained if EARLY_ON else 0), (d, base)


def _assert_frames(order, got, refs, tag=""):
    for k, (c, g) in enumerate(zip(order, got)):
        assert torch.equal(g, refs[c]), f"{tag}frame {k} (camera {c}) differs from the frame rendered alone"


def _hold_back():
    """tens of milliseconds of work on the caller's stream, which the renderers queue behind: heads and cull passes pile up"""
    a = torch.ones(8192, 8192, device=DEV)
    torch.cuda.synchronize()
    b = a @ a
    for _ in range(3):
        b = a @ b
    return b


def _held_burst(lcgs, r, W, H, imgs=None, order=HELD_ORDER):
    """A burst behind _hold_back().  In front of a context's first one, two enqueue-only frames and a synchronisation: they
    create the context's streams and workspace, which can take the host longer than the matrix products run, and the frame
    that pays for them would find the GPU idle; the counts are then asserted from there on (_assert_counts)."""
    cams = _cams(lcgs, W, H)
    if not hasattr(r, "_early_cull_base"):
        _enqueue(r, cams, [torch.full((3, H, W), -1.0, device=DEV)], [0, 1])
        r.ctx.synchronize()
        r._early_cull_base = _counts(r)
    imgs = imgs or [torch.full((3, H, W), -1.0, device=DEV)]
    b = _hold_back()  # noqa: F841
    return _enqueue(r, cams, imgs, order)


# ------------------------------------------------------------------------------------ 1: every cull pass uses its own camera
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_twelve_frames_over_four_cameras_into_one_image(lcgs, size):
    W, H = size
    refs = _refs(lcgs, W, H)
    r = _owned(lcgs, _scene())
    order = [k % 4 for k in range(12)]
    got = _held_burst(lcgs, r, W, H, order=order)
    r.ctx.synchronize()
    _assert_counts(r, 12, 11)  # (the first frame follows a synchronisation: it does not chain, its cull pass stays on the head)
    _assert_frames(order, got, refs)


def test_twelve_frames_with_nothing_in_front(lcgs):
    """the same burst at the GPU's own pace: which frames cull early is a matter of host timing, every image is not"""
    W, H = SIZES[0]
    refs = _refs(lcgs, W, H)
    r = _owned(lcgs, _scene())
    order = [k % 4 for k in range(12)]
    got = _enqueue(r, _cams(lcgs, W, H), [torch.full((3, H, W), -1.0, device=DEV)], order)
    r.ctx.synchronize()
    _assert_counts(r, 12, 11, held=False)
    _assert_frames(order, got, refs)


@pytest.mark.parametrize("policy", ["tile", "block"])
def test_twelve_frames_into_four_rotating_images_per_list_policy(lcgs, policy):
    W, H = SIZES[0]
    refs = _refs(lcgs, W, H, policy)
    r = _owned(lcgs, _scene(), policy)
    imgs = [torch.full((3, H, W), -1.0, device=DEV) for _ in range(4)]
    order = [(3 * k + 1) % 4 for k in range(12)]  # (camera and image rotate differently)
    got = _held_burst(lcgs, r, W, H, imgs, order)
    r.ctx.synchronize()
    _assert_counts(r, 12, 11)
    assert r.frame_stats()["list_shift"] == (1 if policy == "block" else 0)
    _assert_frames(order, got, refs)
    for i in range(4):  # what the images hold at the end: the last frame written to each
        assert torch.equal(imgs[i], refs[order[8 + i]]), i


# --------------------------------------------------------------------- 2: cull passes as far ahead as the events allow
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_held_back_burst_with_repeats_and_empty_views(lcgs, size):
    W, H = size
    refs = _refs(lcgs, W, H)
    r = _owned(lcgs, _scene())
    imgs = [torch.full((3, H, W), -1.0, device=DEV) for _ in range(3)]
    got = _held_burst(lcgs, r, W, H, imgs)
    r.ctx.synchronize()
    _assert_counts(r, 12, 11)
    _assert_frames(HELD_ORDER, got, refs)
    for k, c in enumerate(HELD_ORDER):
        if c == 4:
            assert bool((got[k] == -1.0).all()), f"frame {k}: a view with no survivors drew something (leaked slabs or counts)"


# ----------------------------------------------------------------------- 3: leaving the chain right behind a held-back burst
def test_synchronising_frame_behind_a_held_back_burst(lcgs):
    W, H = SIZES[0]
    refs = _refs(lcgs, W, H)
    r = _owned(lcgs, _scene())
    got = _held_burst(lcgs, r, W, H)
    img, n = _alone(lcgs, r, _cams(lcgs, W, H)[2], W, H)  # (no synchronisation in between)
    assert n > 0 and torch.equal(img, refs[2])
    _assert_frames(HELD_ORDER, got, refs)
    _assert_counts(r, 12, 11)


def _step(lcgs, r, cam, W, H, dL):
    """a keep-state frame and its backward: image, kept state, lists, gradients"""
    img = torch.full((3, H, W), -1.0, device=DEV)
    n = r.forward(cam, img, bg=BG, keep_state=True, sync=True)
    st = r.frame_stats()
    T, nc = torch.zeros(H, W, device=DEV), torch.zeros(H, W, dtype=torch.int32, device=DEV)
    r.last_state(T, nc)
    G = ((W + 15) // 16) * ((H + 15) // 16)
    lst, rng_ = torch.zeros(st["num_pairs"], dtype=torch.int32, device=DEV), torch.zeros(2 * G, dtype=torch.int32, device=DEV)
    r.last_lists(lst, rng_)
    t = r.scene_tensors()
    g = {k: torch.full_like(t[k], 7.0) for k in KEYS}
    r.backward(dL, *[g[k] for k in KEYS])
    r.ctx.synchronize()
    return {"n": n, "img": img, "T": T, "nc": nc, "list": lst, "ranges": rng_, "g": g}


def _step_reference(lcgs, oracle, W, H):
    """the step on a fresh context with nothing around it, its gradient bound (f64 oracle, once), the upstream gradient"""
    def make():
        dL = np.random.default_rng(3).normal(size=(3, H, W)).astype(np.float32)
        r = _owned(lcgs, _scene())
        # (the context keeps its scene in spatial order: the oracle gets the rows in that order)
        scene_rows = {k: v.cpu().numpy() for k, v in r.scene_tensors().items()}
        ocam = oracle.lookat(*POSES[2], width=W, height=H)
        bound = gradient_row_bound(scene_rows, ocam, dL, BG, 1.0, 3, None, None, None, None)
        ref = _step(lcgs, r, _cams(lcgs, W, H)[2], W, H, dev(dL))
        check_gradient_rows(ref["g"], scene_rows, ocam, dL, bg=BG, tag="step alone", bound=bound)
        return ref, bound, dL, scene_rows, ocam
    return cached(("pipelined step", W, H), make)


def test_keep_state_step_behind_a_held_back_burst(lcgs, oracle):
    W, H = SIZES[0]
    ref, bound, dL, scene_rows, ocam = _step_reference(lcgs, oracle, W, H)
    refs = _refs(lcgs, W, H)
    r = _owned(lcgs, _scene())
    got = _held_burst(lcgs, r, W, H)
    a = _step(lcgs, r, _cams(lcgs, W, H)[2], W, H, dev(dL))  # (no synchronisation between the burst and the step)
    _assert_frames(HELD_ORDER, got, refs)
    assert a["n"] == ref["n"]
    for k in ("img", "T", "nc", "list", "ranges"):
        assert torch.equal(a[k], ref[k]), f"the keep-state frame's {k} differs"
    check_gradient_rows(a["g"], scene_rows, ocam, dL, bg=BG, tag="step behind a held-back burst", bound=bound)


def test_frame_with_radii_behind_a_held_back_burst(lcgs):
    W, H = SIZES[0]
    refs = _refs(lcgs, W, H)
    cams = _cams(lcgs, W, H)
    fresh = _owned(lcgs, _scene())
    want = torch.full((P_SCENE,), -7, dtype=torch.int32, device=DEV)
    fresh.forward(cams[3], torch.zeros(3, H, W, device=DEV), bg=BG, radii=want, sync=True)
    r = _owned(lcgs, _scene())
    got = _held_burst(lcgs, r, W, H)
    rad = torch.full((P_SCENE,), -7, dtype=torch.int32, device=DEV)
    img = torch.full((3, H, W), -1.0, device=DEV)
    r.forward(cams[3], img, bg=BG, radii=rad, sync=False)
    r.ctx.synchronize()
    assert torch.equal(img, refs[3]) and torch.equal(rad, want)
    _assert_frames(HELD_ORDER, got, refs)
    _assert_counts(r, 12, 11)


def test_in_place_optimiser_step_behind_a_held_back_burst(lcgs):
    """lcgs_adam_step on the context's own arrays, ordered by the stream alone, right behind a burst whose cull passes ran
    ahead; the four frames behind the step must show the stepped scene, the twelve in front of it the old one."""
    W, H = SIZES[0]
    refs = _refs(lcgs, W, H)
    cams = _cams(lcgs, W, H)
    # (file order, as in test_gpu_pipelined_frames.py: the frames behind the step are compared with a context that BINDS the
    #  stepped arrays, for which the bound order is the file order)
    r = lcgs.Renderer(lcgs.Context(0))
    r.upload_scene(_scene(), order="file")
    act = r.scene_tensors()
    raw = {"pos": act["pos"], "scale": torch.log(act["scale"]), "rotq": act["rotq"].clone(), "sh": act["sh"],
           "opacity": torch.logit(act["opacity"])}
    gen = torch.Generator(device=DEV).manual_seed(7)
    g = {k: torch.randn(raw[k].shape, device=DEV, generator=gen) for k in KEYS}
    m, v = ({k: torch.zeros_like(raw[k]) for k in KEYS} for _ in range(2))
    lr = {"pos": 2e-2, "sh_dc": 5e-2, "sh_rest": 1e-2, "opacity": 3e-1, "scale": 5e-2, "rot": 1e-2}
    torch.cuda.synchronize()
    img = torch.full((3, H, W), -1.0, device=DEV)
    got_a = _held_burst(lcgs, r, W, H, [img])
    r.adam_step(g, raw, m, v, act, 1, lr)
    behind = [3, 0, 1, 2]
    got_b = _enqueue(r, cams, [img], behind)
    r.ctx.synchronize()
    _assert_counts(r, 12, 11)  # (the step drops the context's derived cull rows: the frames behind it leave the head stream)
    _assert_frames(HELD_ORDER, got_a, refs, "in front of the step: ")
    fresh = lcgs.Renderer(lcgs.Context(0))
    stepped = {k: act[k].clone() for k in KEYS}
    fresh.bind_scene(*[stepped[k] for k in KEYS])
    for c, x in zip(behind, got_b):
        want, _ = _alone(lcgs, fresh, cams[c], W, H)
        assert not torch.equal(want, refs[c])  # the step is visible
        assert torch.equal(x, want), f"camera {c}: a frame behind the step does not show the stepped scene"


# ------------------------------------------------------------------------------------------------ 4: a scene of another size
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scene_of_another_size_behind_a_burst(lcgs, size):
    W, H = size
    refs, small = _refs(lcgs, W, H), _small_refs(lcgs, W, H)
    r = _owned(lcgs, _scene())
    got_a = _held_burst(lcgs, r, W, H)
    r.upload_scene(_small_scene())  # three chunks instead of ten: the table's row stride and the slabs in use change
    got_b = _held_burst(lcgs, r, W, H)
    r.ctx.synchronize()
    _assert_counts(r, 24, 22)  # the frame behind the upload does not chain
    _assert_frames(HELD_ORDER, got_a, refs, "first scene: ")
    _assert_frames(HELD_ORDER, got_b, small, "second scene: ")


# ---------------------------------------------------------------------------------------------------------- 5: the switch
@pytest.mark.parametrize("switch", ["LCGS_EARLY_CULL", "LCGS_PIPELINE"])
def test_every_case_again_with_the_switch_off(switch):
    env = dict(os.environ, **{switch: "0"})
    me = "tests/test_gpu_early_cull.py"
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", me,
                          "-k", "not test_every_case_again_with_the_switch_off"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
