"""`-m gpu`: pipelined in-order frames.  Forward-only frames enqueued without read-back run their head -- cull,
depth sort, duplication, tile partition, ranges -- on the context's head stream, beside the previous frame's renderer.  Every
image must still be the image of its own camera and scene, written in stream order: each comparison here is bit equality
(torch.equal) with the same frame rendered alone by a synchronising call on a fresh context, which is the single-stream path
the other suites hold to the oracle; one pipelined frame is held to the oracle directly.

The whole file runs a second time in a child process under LCGS_PIPELINE=0 (the hook is read when a context is created),
where every frame takes the single-stream order.

Gradients behind pipelined frames: the render-backward adds floats with atomics, so two runs of one and the same step differ
in their last bits and cannot be compared with torch.equal.  What the backward READS is deterministic, and is compared
exactly -- the keep-state frame's image, its kept final transmittance and last-contributor map, its per-tile lists and
ranges --, and the gradients themselves are held row by row to the suite's bound against the f64 oracle
(gpu_util.check_gradient_rows), with and without pipelined frames around the step."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, make_scene
from gpu_util import DEV, KEYS, assert_image_parity, cached, check_gradient_rows, dev, gradient_row_bound, upload_scene

pytestmark = pytest.mark.gpu

BG = (0.1, 0.2, 0.3)
P_SCENE = 20000
# four views of the scene, and one turned away from it (nothing on screen)
POSES = [([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1]), ([2.5, -2.0, 1.2], [0, 0, 0.5], [0, 0, 1]),
         ([0.3, 3.2, 0.9], [0, 0, 0.5], [0, 0, 1]), ([-1.5, -2.8, 3.0], [0.2, 0.1, 0.4], [0, 0, 1])]
AWAY = ([-3, -0.5, 2.3], [-6, -1.0, 4.1], [0, 0, 1])
SIZES = [(256, 144), (250, 130)]  # 16 x 9 tiles (an odd tile row: a half block); partial tiles right and below


def _scene(seed=5):
    return cached(("pipelined scene", seed), lambda: make_scene(np.random.default_rng(seed), P_SCENE))


def _cams(lcgs, W, H, poses=POSES):
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
        out = [_alone(lcgs, r, c, W, H) for c in _cams(lcgs, W, H, POSES + [AWAY])]
        assert all(n > 0 for _, n in out[:4]) and out[4][1] == 0 and bool((out[4][0] == -1.0).all())
        assert not any(torch.equal(out[i][0], out[j][0]) for i in range(4) for j in range(i))  # four different images
        return [img for img, _ in out]
    return cached(("pipelined refs", W, H, policy, seed), make)


def _enqueue(r, cams, imgs, order, clones=True):
    """frames order[k] -> imgs[k % len(imgs)] without read-back; the image is cloned on the stream behind each call"""
    out = []
    for k, c in enumerate(order):
        img = imgs[k % len(imgs)]
        r.forward(cams[c], img, bg=BG, sync=False)
        if clones:
            out.append(img.clone())
    return out


def _assert_chained(r, frames, chained):
    """what the context itself says it did (lcgs_debug_pipeline_counts): without this a library that never chained -- or
    never used the head stream at all -- would pass every comparison below"""
    pc = r.pipeline_counts()
    if os.environ.get("LCGS_PIPELINE") == "0":
        assert pc == {"piped": 0, "chained": 0, "bounded": 0}, pc
    else:
        assert pc["piped"] == frames and pc["chained"] == chained, pc


# ---------------------------------------------------------------------------------------------------- 1, 2: plain runs
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_twelve_frames_over_four_cameras_into_one_image(lcgs, size):
    W, H = size
    refs = _refs(lcgs, W, H)
    r = _owned(lcgs, _scene())
    img = torch.full((3, H, W), -1.0, device=DEV)
    order = [k % 4 for k in range(12)]
    got = _enqueue(r, _cams(lcgs, W, H), [img], order)
    r.ctx.synchronize()
    _assert_chained(r, 12, 11)  # (the first frame follows the upload: its head waits for the caller's stream)
    for k, (c, g) in enumerate(zip(order, got)):
        assert torch.equal(g, refs[c]), f"frame {k} (camera {c}) differs from the frame rendered alone"


def test_chained_frames_with_the_bounded_renderer_grid_at_1080p(lcgs):
    """A frame that chains while the GPU is behind the host renders with a bounded persistent grid (3 workgroups per CU), which
    only exists where a frame has more tiles than that: 1080p, 8160 tiles.  A long matrix product on the stream in front
    holds the first renderer back, so that every later frame finds its predecessor's renderer unfinished."""
    W, H = 1920, 1080
    cams = _cams(lcgs, W, H)[:2]
    fresh = _owned(lcgs, _scene())
    refs = [_alone(lcgs, fresh, c, W, H)[0] for c in cams]
    assert not torch.equal(refs[0], refs[1])
    r = _owned(lcgs, _scene())
    imgs = [torch.full((3, H, W), -1.0, device=DEV) for _ in range(2)]
    a = torch.ones(8192, 8192, device=DEV)
    torch.cuda.synchronize()
    b = a @ a  # noqa: F841 (tens of milliseconds of work the renderers queue behind)
    order = [0, 1, 1, 0, 1, 0, 0, 1]
    got = _enqueue(r, cams, imgs, order)
    r.ctx.synchronize()
    _assert_chained(r, 8, 7)
    if os.environ.get("LCGS_PIPELINE") != "0":
        assert r.pipeline_counts()["bounded"] == 7, r.pipeline_counts()
    for k, (c, g) in enumerate(zip(order, got)):
        assert torch.equal(g, refs[c]), f"frame {k} (camera {c}) differs from the frame rendered alone"


def test_one_pipelined_frame_against_the_oracle(lcgs, oracle):
    W, H = SIZES[0]
    r = _owned(lcgs, _scene())
    img = torch.full((3, H, W), -1.0, device=DEV)
    got = _enqueue(r, _cams(lcgs, W, H), [img], [0, 1, 2, 3, 0, 1])
    r.ctx.synchronize()
    orc = oracle.render(_scene(), oracle.lookat(*POSES[0], width=W, height=H), bg=BG, ambig_eps=1e-5)
    assert_image_parity(got[4].cpu().numpy(), orc)  # the fifth frame: chained behind four others, one more behind it
    assert r.frame_stats()["num_rendered"] == oracle.render(_scene(), oracle.lookat(*POSES[1], width=W, height=H), bg=BG,
                                                            ambig_eps=1e-5)["num_rendered"]


@pytest.mark.parametrize("policy", ["tile", "block"])
def test_twelve_frames_into_four_rotating_images_per_list_granularity(lcgs, policy):
    W, H = SIZES[0]
    refs = _refs(lcgs, W, H, policy)
    r = _owned(lcgs, _scene(), policy)
    imgs = [torch.full((3, H, W), -1.0, device=DEV) for _ in range(4)]
    order = [(3 * k + 1) % 4 for k in range(12)]  # (camera and image rotate differently)
    got = _enqueue(r, _cams(lcgs, W, H), imgs, order)
    r.ctx.synchronize()
    assert r.frame_stats()["list_shift"] == (1 if policy == "block" else 0)
    for k, (c, g) in enumerate(zip(order, got)):
        assert torch.equal(g, refs[c]), f"frame {k} (camera {c}) differs"
    for i in range(4):  # what the images hold at the end: the last frame written to each
        assert torch.equal(imgs[i], refs[order[8 + i]]), i


# ------------------------------------------------------------------------------------------ 3: ordering against other work
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


def _same_step(a, ref):
    assert a["n"] == ref["n"]
    for k in ("img", "T", "nc", "list", "ranges"):
        assert torch.equal(a[k], ref[k]), f"the keep-state frame's {k} differs"


def test_keep_state_step_behind_pipelined_frames(lcgs, oracle):
    W, H = SIZES[0]
    ref, bound, dL, scene_rows, ocam = _step_reference(lcgs, oracle, W, H)
    refs = _refs(lcgs, W, H)
    r = _owned(lcgs, _scene())
    img = torch.full((3, H, W), -1.0, device=DEV)
    got = _enqueue(r, _cams(lcgs, W, H), [img], [0, 1, 3, 0, 1])
    a = _step(lcgs, r, _cams(lcgs, W, H)[2], W, H, dev(dL))  # (no synchronisation between the frames and the step)
    for c, g in zip([0, 1, 3, 0, 1], got):
        assert torch.equal(g, refs[c])
    _same_step(a, ref)
    check_gradient_rows(a["g"], scene_rows, ocam, dL, bg=BG, tag="step behind pipelined frames", bound=bound)


def test_pipelined_frames_behind_a_keep_state_step(lcgs, oracle):
    W, H = SIZES[0]
    ref, bound, dL, scene_rows, ocam = _step_reference(lcgs, oracle, W, H)
    refs = _refs(lcgs, W, H)
    r = _owned(lcgs, _scene())
    cams = _cams(lcgs, W, H)
    # the step WITHOUT its trailing synchronisation: the frames follow a backward that still reads the workspace
    kimg = torch.full((3, H, W), -1.0, device=DEV)
    r.forward(cams[2], kimg, bg=BG, keep_state=True, sync=False)
    t = r.scene_tensors()
    g = {k: torch.full_like(t[k], 7.0) for k in KEYS}
    r.backward(dev(dL), *[g[k] for k in KEYS])
    img = torch.full((3, H, W), -1.0, device=DEV)
    got = _enqueue(r, cams, [img], [1, 0, 3, 1])
    r.ctx.synchronize()
    assert torch.equal(kimg, ref["img"])
    for c, x in zip([1, 0, 3, 1], got):
        assert torch.equal(x, refs[c])
    check_gradient_rows(g, scene_rows, ocam, dL, bg=BG, tag="step in front of pipelined frames", bound=bound)


def test_last_lists_and_frame_stats_behind_pipelined_frames(lcgs):
    W, H = SIZES[0]
    G = ((W + 15) // 16) * ((H + 15) // 16)
    cams = _cams(lcgs, W, H)

    def lists(r):
        st = r.frame_stats()
        lst, rng_ = torch.zeros(st["num_pairs"], dtype=torch.int32, device=DEV), torch.zeros(2 * G, dtype=torch.int32, device=DEV)
        r.last_lists(lst, rng_)
        return st, lst, rng_

    fresh = _owned(lcgs, _scene(), "tile")
    _alone(lcgs, fresh, cams[3], W, H)
    want = lists(fresh)
    for frames in ([3], [0, 3], [0, 1, 3], [0, 1, 2, 3]):  # the last frame ends in each of the pair-value buffers
        r = _owned(lcgs, _scene(), "tile")
        _enqueue(r, cams, [torch.zeros(3, H, W, device=DEV)], frames, clones=False)
        st, lst, rng_ = lists(r)
        assert st == want[0], (frames, st, want[0])
        assert torch.equal(lst, want[1]) and torch.equal(rng_, want[2]), frames


def test_scene_writer_between_pipelined_frames(lcgs):
    W, H = SIZES[0]
    refs_a, refs_b = _refs(lcgs, W, H), _refs(lcgs, W, H, seed=6)
    assert not torch.equal(refs_a[0], refs_b[0])
    r = _owned(lcgs, _scene())
    cams = _cams(lcgs, W, H)
    img = torch.full((3, H, W), -1.0, device=DEV)
    got_a = _enqueue(r, cams, [img], [0, 1, 2])
    r.upload_scene(_scene(6))  # a library writer of the context's scene
    got_b = _enqueue(r, cams, [img], [2, 0, 1])
    r.ctx.synchronize()
    _assert_chained(r, 6, 4)  # the frame behind the upload does not chain
    for c, g in zip([0, 1, 2], got_a):
        assert torch.equal(g, refs_a[c])
    for c, g in zip([2, 0, 1], got_b):
        assert torch.equal(g, refs_b[c]), "a frame behind the upload shows the old scene"


def test_in_place_optimiser_step_between_pipelined_frames(lcgs):
    """lcgs_adam_step on the context's own arrays: an in-place writer that is only ordered by the stream (no reallocation, no
    synchronisation, unlike the upload above).  The frames behind it must show the stepped scene: their heads may not run
    ahead of the step on the caller's stream.  (The step drops the context's derived cull rows, so those frames also leave the
    head stream until the scene is bound again: the counts stay where the frames in front left them.)"""
    W, H = SIZES[0]
    refs = _refs(lcgs, W, H)
    cams = _cams(lcgs, W, H)
    # (file order: the frames behind the step are compared with a context that BINDS the stepped arrays, for which the bound
    #  order is the file order -- equal depths, which 20 000 splats do have, blend in file order)
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
    got_a = _enqueue(r, cams, [img], [0, 1, 2, 3])
    r.adam_step(g, raw, m, v, act, 1, lr)
    got_b = _enqueue(r, cams, [img], [3, 0, 1])
    r.ctx.synchronize()
    _assert_chained(r, 4, 3)
    for c, x in zip([0, 1, 2, 3], got_a):
        assert torch.equal(x, refs[c]), "a frame in front of the step shows the stepped scene"
    fresh = lcgs.Renderer(lcgs.Context(0))
    stepped = {k: act[k].clone() for k in KEYS}
    fresh.bind_scene(*[stepped[k] for k in KEYS])
    for c, x in zip([3, 0, 1], got_b):
        want, _ = _alone(lcgs, fresh, cams[c], W, H)
        assert not torch.equal(want, refs[c])  # the step is visible
        assert torch.equal(x, want), (f"camera {c}: a frame behind the step does not show the stepped scene: "
                                      f"{int((x != want).any(0).sum())} pixels differ, {int((x != refs[c]).any(0).sum())} from the old scene")


def test_caller_bound_arrays_written_in_place_between_frames(lcgs):
    W, H = SIZES[0]
    cams = _cams(lcgs, W, H)
    d = upload_scene(_scene())
    r = lcgs.Renderer(lcgs.Context(0))
    r.bind_scene(*[d[k] for k in KEYS])  # caller-owned, not declared static: torch may write them between frames
    # (such frames never use the head stream: asserted at the end)
    img = torch.full((3, H, W), -1.0, device=DEV)
    got, states = [], []
    for k in range(6):
        r.forward(cams[k % 2], img, bg=BG, sync=False)
        got.append(img.clone())
        states.append({key: d[key].clone() for key in ("pos", "opacity")})
        d["opacity"].mul_(0.8)  # on the stream, behind the frame that must not see it
        d["pos"][:, 2].add_(0.05)
    r.ctx.synchronize()
    fresh = lcgs.Renderer(lcgs.Context(0))
    for k in range(6):
        fresh.bind_scene(states[k]["pos"], d["scale"], d["rotq"], d["sh"], states[k]["opacity"])
        want, _ = _alone(lcgs, fresh, cams[k % 2], W, H)
        assert torch.equal(got[k], want), f"frame {k} does not show the arrays as they were when it was enqueued"
    assert not torch.equal(got[0], got[2])
    assert r.pipeline_counts() == {"piped": 0, "chained": 0, "bounded": 0}


def test_frames_with_radii_between_frames_without(lcgs):
    W, H = SIZES[0]
    refs = _refs(lcgs, W, H)
    cams = _cams(lcgs, W, H)
    fresh = _owned(lcgs, _scene())
    want_radii = []
    for c in range(4):
        rad = torch.full((P_SCENE,), -7, dtype=torch.int32, device=DEV)
        fresh.forward(cams[c], torch.zeros(3, H, W, device=DEV), bg=BG, radii=rad, sync=True)
        want_radii.append(rad)
    r = _owned(lcgs, _scene())
    img = torch.full((3, H, W), -1.0, device=DEV)
    got, got_radii = [], {}
    order = [0, 1, 2, 3, 1, 0, 3, 2, 0, 1]
    for k, c in enumerate(order):
        rad = torch.full((P_SCENE,), -7, dtype=torch.int32, device=DEV) if k in (2, 5, 6, 9) else None
        r.forward(cams[c], img, bg=BG, radii=rad, sync=False)
        got.append(img.clone())
        if rad is not None:
            got_radii[k] = rad
    r.ctx.synchronize()
    for k, c in enumerate(order):
        assert torch.equal(got[k], refs[c]), k
    for k, rad in got_radii.items():
        assert torch.equal(rad, want_radii[order[k]]), k


# ------------------------------------------------------------------------------------------- 4: a frame that renders nothing
def test_view_that_renders_nothing_between_two_views(lcgs):
    W, H = SIZES[0]
    refs = _refs(lcgs, W, H)
    cams = _cams(lcgs, W, H, POSES + [AWAY])
    r = _owned(lcgs, _scene())
    imgs = [torch.full((3, H, W), -1.0, device=DEV) for _ in range(4)]
    order = [0, 1, 4, 2, 4, 4, 3, 0]
    got = _enqueue(r, cams, imgs, order)
    r.ctx.synchronize()
    # frame k goes to image k % 4: cameras 0, 1, none, 2 into images 0..3, then none, none, 3, 0
    assert torch.equal(got[0], refs[0]) and torch.equal(got[1], refs[1]) and torch.equal(got[3], refs[2])
    assert bool((got[2] == -1.0).all()), "an image nothing was drawn into has been written"
    assert torch.equal(got[4], refs[0]) and torch.equal(got[5], refs[1])  # images 0 and 1 behind an empty view each: untouched
    assert torch.equal(got[6], refs[3]) and torch.equal(got[7], refs[0])
    assert torch.equal(imgs[0], refs[0]) and torch.equal(imgs[1], refs[1])


# ------------------------------------------------------------------------------------------------- 5: pair-capacity overflow
def test_overflow_of_pipelined_frames_is_reported_at_the_next_sync(lcgs):
    """The pair workspace starts at max(4 P, 2^22) pairs whatever the test's resolution, so this case alone runs at 1080p, with
    6000 big splats and per-tile lists (tests/test_gpu_fused.py's overflow scene)."""
    W, H = 1920, 1080
    scene = cached("pipelined overflow scene", lambda: make_scene(np.random.default_rng(13), 6000, log_scale=(-1.0, 0.2)))
    big = lcgs.get_lookat_cam(*POSES[0], width=W, height=H)
    sliver = lcgs.get_lookat_cam([-3, -0.5, 2.3], [-4.5, 2.0, 2.2], [0, 0, 1], width=W, height=H)  # the scene at the frame's edge
    r = _owned(lcgs, scene, "tile")
    img = torch.zeros(3, H, W, device=DEV)
    n_sliver = r.forward(sliver, img, bg=BG, sync=True)
    imgs = [torch.zeros(3, H, W, device=DEV) for _ in range(3)]
    _enqueue(r, [big], imgs, [0, 0, 0], clones=False)
    with pytest.raises(lcgs.LcgsError) as e:
        r.ctx.synchronize()
    assert e.value.status == 5 and "truncated" in str(e.value) and "3 asynchronous" in str(e.value)  # LCGS_ERR_CAPACITY
    r.ctx.synchronize()  # reported once, then clear; the workspace has been grown
    _enqueue(r, [big], imgs, [0, 0, 0], clones=False)
    r.ctx.synchronize()
    fresh = _owned(lcgs, scene, "tile")
    want = torch.zeros(3, H, W, device=DEV)
    n = fresh.forward(big, want, bg=BG, sync=True)
    assert n > (1 << 22) and n_sliver < n // 4
    for i in range(3):
        assert torch.equal(imgs[i], want), i


# ------------------------------------------------------------------------------- 6: everything again in single-stream order
def test_every_case_again_with_the_pipeline_switched_off():
    env = dict(os.environ, LCGS_PIPELINE="0")
    me = "tests/test_gpu_pipelined_frames.py"
    res = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", me,
                          "--deselect", me + "::test_every_case_again_with_the_pipeline_switched_off"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
