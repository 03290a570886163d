"""`-m gpu`: every kernel of lcgs_adam_step (csrc/kernels/train.hip) held per element to the float64 restatement of its
contract, tests/adam_ref.py: |kernel - step64| <= 2 x the first-order rounding bound on raw, m, v AND the activated arrays, one
step from a given random state (the inputs are exact and the bound a priori).  tests/test_adam_ref.py pins the yardstick on the
CPU; docs/TESTS.md "Optimiser step" has the measured ratios and the mutants this file was shown to catch."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import adam_ref as R
from conftest import make_scene
from gpu_util import DEV

pytestmark = pytest.mark.gpu

KEYS, ARRAYS = R.KEYS, R.ARRAYS
PS = (1, 255, 256, 257, 20011)
# train.hip::grid_for: 256 work items per block, at most 65 536 blocks -- more work items than this and the loops wrap
WORK_ITEMS_CAP = 65536 * 256


def _cases():
    """(aliased, degree, P, step, eps): every P, step and eps against both aliasings and degrees 0 and 3; degrees 1 and 2 against
    both aliasings"""
    out = []
    for aliased in (True, False):
        for deg in (0, 3):
            for i, (P, step) in enumerate(zip(PS, R.STEPS)):
                out.append((aliased, deg, P, step, R.EPSES[(i + deg + aliased) % 2]))
        out += [(aliased, 1, 257, 10, R.EPSES[aliased]), (aliased, 2, 255, 2, R.EPSES[1 - aliased])]
    for aliased in (True, False):
        for deg in (0, 3):
            mine = [c for c in out if c[0] == aliased and c[1] == deg]
            assert {c[2] for c in mine} == set(PS) and {c[3] for c in mine} == set(R.STEPS) and {c[4] for c in mine} == set(R.EPSES)
    return out


CASES = _cases()
# the one-step test: every case x every class.  The saturation class is defined at eps = 1e-15 (eps against sqrt(v') c2), so its
# cases carry that eps whatever the case's own: they still differ from one another in aliasing, degree, P and step
ONE_STEP = [(*c[:4], 1e-15 if cls == "saturation" else c[4], cls) for c in CASES for cls in R.CLASSES]


def _to(pack, device):
    return {k: t.to(device) for k, t in pack.items()}


def _adam(lcgs, r, deg, g, raw, m, v, act, s, visible_only=0):
    """one lcgs_adam_step in place: degree 3 through the binding, the others straight through the C ABI"""
    if deg == 3:
        r.adam_step(g, raw, m, v, act, s["step"], s["lr"], betas=(s["b1"], s["b2"]), eps=s["eps"],
                    visible_only=visible_only != 0, compact_grads=visible_only == 2)
    else:
        lr = s["lr"]
        cfg = lcgs.api._AdamConfig(lr["pos"], lr["sh_dc"], lr["sh_rest"], lr["opacity"], lr["scale"], lr["rot"], s["b1"], s["b2"],
                                   s["eps"], s["step"], visible_only)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        grads = lcgs.api._Grads(*[ptr(g[k]) for k in KEYS])
        packs = [lcgs.api._Params(*[ptr(d[k]) for k in KEYS]) for d in (raw, m, v, act)]
        st = lcgs.load_library().lcgs_adam_step(r.ctx._h, int(raw["pos"].shape[0]), deg, C.byref(cfg), C.byref(grads),
                                                *[C.byref(p) for p in packs])
        assert st == 0, lcgs.load_library().lcgs_last_error()
    r.ctx.synchronize()


def _step(lcgs, r, deg, inp, s, aliased, visible_only=0, wrap=None):
    """the kernels on device copies of `inp` -> {"raw", "m", "v", "act"} of device packs.  aliased: activated pos / sh ARE raw's;
    wrap: applied to the five SH tensors (the unaligned views)"""
    g, raw, m, v, act = [{k: t.to(DEV).clone() for k, t in p.items()} for p in inp]
    if wrap is not None:
        for p in (g, raw, m, v, act):
            p["sh"] = wrap(p["sh"])
    if aliased:
        assert torch.equal(act["pos"], raw["pos"]) and torch.equal(act["sh"], raw["sh"])
        act["pos"], act["sh"] = raw["pos"], raw["sh"]
    else:
        assert act["pos"].data_ptr() != raw["pos"].data_ptr() and act["sh"].data_ptr() != raw["sh"].data_ptr()
    _adam(lcgs, r, deg, g, raw, m, v, act, s, visible_only)
    return {"raw": raw, "m": m, "v": v, "act": act}


def _assert_bound(got, inp, s, tag, rows=None, compact=False):
    res = R.check(got, *inp, s, rows=rows, compact=compact)
    R.report(res, tag)
    assert not R.failures(res), (tag, R.failures(res))
    return res


@pytest.fixture(scope="module")
def renderer(lcgs):
    return lcgs.Renderer(lcgs.Context(0))


@pytest.mark.parametrize("aliased,deg,P,step,eps,cls", ONE_STEP)
def test_one_step_meets_the_bound(lcgs, renderer, aliased, deg, P, step, eps, cls):
    s = R.scalars(step, eps=eps)
    F = 3 * (deg + 1) ** 2
    inp = R.make_inputs(cls, P, F, 7919 * P + 31 * step + deg, s)
    got = {a: _to(p, "cpu") for a, p in _step(lcgs, renderer, deg, inp, s, aliased).items()}
    tag = f"{cls} P={P} degree={deg} step={step} eps={s['eps']:.0e} {'aliased' if aliased else 'separate'}"
    _assert_bound(got, inp, s, tag)
    # a measurement, not an assertion: how many elements differ from the float32 restatement
    r32 = R.step32(*inp, s)
    print(f"[adam] {tag}: elements != step32 (pos/scale/rotq/sh/opacity)  " + "  ".join(
        f"{a} " + "/".join(str(int((got[a][k] != r32[a][k]).sum())) for k in KEYS) for a in ARRAYS))
    for k in ("pos", "sh"):
        assert torch.equal(got["act"][k], got["raw"][k]), k  # identity activation: the same float in both arrays


@pytest.mark.parametrize("aliased,deg,P,step,eps", [c for c in CASES if c[2] in (1, 257)])
def test_zero_rows_stay_bit_for_bit(lcgs, renderer, aliased, deg, P, step, eps):
    """g = m = v = 0: raw, m, v and the activated arrays unchanged, the activated arrays being the kernels' own (the output of
    a first such step)"""
    s = R.scalars(step, eps=eps)
    _, raw, _, _, act = R.make_inputs("general", P, 3 * (deg + 1) ** 2, P + step, s)
    zero = {k: torch.zeros_like(t) for k, t in raw.items()}
    first = _step(lcgs, renderer, deg, (zero, raw, zero, zero, act), s, aliased)
    again = _step(lcgs, renderer, deg, (zero, first["raw"], first["m"], first["v"], first["act"]), s, aliased)
    for a in ARRAYS:
        for k in KEYS:
            assert torch.equal(first[a][k], again[a][k]), (a, k)
            if a != "act":
                assert torch.equal(first[a][k].cpu(), (raw if a == "raw" else zero)[k]), (a, k)
    for k in ("scale", "rotq", "opacity"):  # ... and they are activations of raw
        assert torch.allclose(first["act"][k].cpu(), act[k], rtol=1e-6, atol=0), k


def _one_float_in(t):
    """the same values as a view that starts one float into a larger allocation"""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


@pytest.mark.parametrize("P", [257, 20011])
def test_unaligned_degree3_sh_takes_the_row_kernel(lcgs, renderer, P):
    """k_adam_rows<48, 0>: the five SH pointers 4 bytes past a 16-byte boundary.  Inside the bound, and the aligned call's bits:
    the same adam_update, built without FMA contraction."""
    s = R.scalars(10, eps=1e-15)
    inp = R.make_inputs("general", P, 48, P, s)
    got = _step(lcgs, renderer, 3, inp, s, aliased=False, wrap=_one_float_in)
    assert all(got[a]["sh"].data_ptr() % 16 == 4 for a in ARRAYS)
    aligned = _step(lcgs, renderer, 3, inp, s, aliased=False)
    assert all(aligned[a]["sh"].data_ptr() % 16 == 0 for a in ARRAYS)
    _assert_bound({a: _to(p, "cpu") for a, p in got.items()}, inp, s, f"unaligned SH P={P}")
    for a in ARRAYS:
        for k in KEYS:
            assert torch.equal(got[a][k], aligned[a][k]), (a, k)


def _grid_stride_case(lcgs, renderer, P, deg, wrap, tag):
    """general class, generated and checked in float64 ON THE DEVICE; only the worst ratios and the counts come back"""
    t0 = time.perf_counter()
    s = R.scalars(1000, eps=1e-15)
    inp = R.make_inputs("general", P, 3 * (deg + 1) ** 2, P, s, device=DEV)
    got = _step(lcgs, renderer, deg, inp, s, aliased=wrap is None, wrap=wrap)
    if wrap is not None:
        assert all(got[a]["sh"].data_ptr() % 16 == 4 for a in ARRAYS)
    _assert_bound(got, inp, s, tag)
    # the rows behind the first pass of the loops moved
    for k in KEYS:
        assert not torch.equal(got["m"][k][-1], inp[2][k][-1].to(DEV)), k
    torch.cuda.synchronize()
    print(f"[adam] {tag}: {time.perf_counter() - t0:.1f} s")


@pytest.mark.parametrize("unaligned", [False, True])
def test_grid_stride_degree3(lcgs, renderer, unaligned):
    """k_adam_sh48's loop wraps (16-byte items, twelve per row: four rows lie behind the first pass); on unaligned views
    k_adam_rows<48> wraps"""
    P = 1_398_105
    assert 12 * P > WORK_ITEMS_CAP >= 12 * (P - 4) and 48 * P > WORK_ITEMS_CAP
    _grid_stride_case(lcgs, renderer, P, 3, _one_float_in if unaligned else None,
                      f"grid-stride degree 3 P={P} {'unaligned' if unaligned else 'aligned'}")


def test_grid_stride_degree0(lcgs, renderer):
    """P rows > the cap: k_adam_rot and k_adam_rows<1> (one item per row) wrap, k_adam_rows<3> (pos, scale, degree-0 SH) passes
    four times.  0.94 GB per pack."""
    P = 16_777_473
    assert P > WORK_ITEMS_CAP and -(-3 * P // WORK_ITEMS_CAP) == 4
    _grid_stride_case(lcgs, renderer, P, 0, None, f"grid-stride degree 0 P={P}")


@pytest.fixture(scope="module")
def culled_frame(lcgs):
    """the 4000-splat scene with 1500 culled rows and the 128 x 96 frame of test_adam_visible_only_touches_survivors_only"""
    rng = np.random.default_rng(3)
    P = 4000
    scene = make_scene(rng, P)
    scene["pos"][:1500] += 100.0
    dev = {k: torch.from_numpy(np.ascontiguousarray(scene[k], dtype=np.float32)).to(DEV) for k in KEYS}
    r = lcgs.Renderer(lcgs.Context(0))
    r.bind_scene(*[dev[k] for k in KEYS])
    cam = lcgs.get_lookat_cam([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1], width=128, height=96)
    r.forward(cam, torch.zeros(3, 96, 128, device=DEV), keep_state=True, sync=True)
    rows = r.visible_rows().long().cpu()
    assert rows.numel() == r.frame_stats()["num_visible"] and 0 < rows.numel() <= P - 1500 and int(rows.min()) >= 1500
    yield r, P, rows  # (the bound arrays `dev` stay alive for as long as the fixture does)


@pytest.mark.parametrize("mode", [1, 2])
def test_visible_only_rows_meet_the_bound_and_the_others_are_untouched(lcgs, culled_frame, mode):
    """synthetic general-class gradients and state (no backward: its float atomics have no business here) on the frame's row list:
    dense-indexed gradients (1), then compact ones holding only V rows (2)"""
    r, P, rows = culled_frame
    s = R.scalars(10, eps=1e-15)
    inp = R.make_inputs("general", P, 48, 40 + mode, s)
    if mode == 2:
        inp = ({k: t[rows].clone() for k, t in inp[0].items()},) + inp[1:]
        assert all(t.shape[0] == rows.numel() for t in inp[0].values())
    got = {a: _to(p, "cpu") for a, p in _step(lcgs, r, 3, inp, s, aliased=True, visible_only=mode).items()}
    _assert_bound(got, inp, s, f"visible_only={mode} V={rows.numel()}", rows=rows, compact=mode == 2)
    off = torch.ones(P, dtype=torch.bool)
    off[rows] = False
    for a, start in zip(ARRAYS, inp[1:]):
        for k in KEYS:
            assert torch.equal(got[a][k][off], start[k][off]), (a, k)
            assert not torch.equal(got[a][k][rows], start[k][rows]), (a, k)


def test_fifty_steps_on_the_kernels_own_state(lcgs, renderer):
    """P = 257, degree 3, fresh gradients each step, from zero moments.  The state is the kernels' own after step 1, so the bar
    is the photometric suite's, per array: 3 E32 + 4 u S (adam_ref.trajectory_bound)."""
    P, gen = 257, torch.Generator().manual_seed(50)
    n = lambda shape, mu, sd: (mu + sd * torch.randn(shape, generator=gen, dtype=torch.float64)).float()
    raw0 = {k: n(shape, mu, sd) for (k, shape), (mu, sd) in zip(R.shapes(P, 48).items(), ((0, 1), (-4, 1), (0, 1), (0, 0.3), (0, 2)))}
    grads = [{k: (torch.randn(t.shape, generator=gen, dtype=torch.float64)
                  * 10.0 ** (-4.0 * torch.rand((), generator=gen, dtype=torch.float64))).float() for k, t in raw0.items()}
             for _ in range(50)]
    t64, t32 = R.trajectory(raw0, grads, torch.float64), R.trajectory(raw0, grads, torch.float32)
    raw = _to(raw0, DEV)
    act = {k: t.clone() for k, t in _to(R.activate32(raw0), DEV).items()}
    act["pos"], act["sh"] = raw["pos"], raw["sh"]
    m = {k: torch.zeros_like(t) for k, t in raw.items()}
    v = {k: torch.zeros_like(t) for k, t in raw.items()}
    for step, g in enumerate(grads, 1):
        _adam(lcgs, renderer, 3, _to(g, DEV), raw, m, v, act, R.scalars(step))
    worst = {}
    for a, pack in zip(ARRAYS, (raw, m, v, act)):
        for k in KEYS:
            diff = float((pack[k].cpu().double() - t64[a][k]).abs().max())
            worst[(a, k)] = diff / R.trajectory_bound(t64[a][k], t32[a][k])
    print("[adam] 50 steps: worst diff / (3 E32 + 4 u S)  " + "  ".join(
        f"{a} " + "/".join(f"{worst[(a, k)]:.3f}" for k in KEYS) for a in ARRAYS))
    assert all(x <= 1.0 for x in worst.values()), {k: x for k, x in worst.items() if not x <= 1.0}
