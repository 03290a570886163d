"""`-m gpu`: the optimiser step behind the backward against torch's own autograd + Adam on the CPU,
and the torch autograd binding of the frame against the oracle backward."""
import numpy as np
import pytest
import torch

import adam_ref
from conftest import make_scene
from gpu_util import DEV, check_gradient_rows, gradient_row_bound

pytestmark = pytest.mark.gpu

KEYS = ("pos", "scale", "rotq", "sh", "opacity")
LR = {"pos": 1.6e-4, "sh_dc": 2.5e-3, "sh_rest": 1.25e-4, "opacity": 5e-2, "scale": 5e-3, "rot": 1e-3}


def _activate(raw):
    return {"pos": raw["pos"], "scale": torch.exp(raw["scale"]),
            "rotq": raw["rotq"] / raw["rotq"].norm(dim=1, keepdim=True), "sh": raw["sh"],
            "opacity": torch.sigmoid(raw["opacity"])}


def _torch_reference(raw0, grads_seq, eps):
    """torch.optim.Adam on the raw parameters, gradients w.r.t. the activated values pushed through autograd."""
    raw = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in raw0.items()}
    dc_mask = torch.zeros(48, dtype=torch.float64)
    dc_mask[:3] = 1.0
    # SH has two learning rates (dc, rest): two parameter tensors behind one activated array
    sh_dc = (raw["sh"].detach()[:, :3]).clone().requires_grad_(True)
    sh_rest = (raw["sh"].detach()[:, 3:]).clone().requires_grad_(True)
    groups = [{"params": [raw["pos"]], "lr": LR["pos"]}, {"params": [sh_dc], "lr": LR["sh_dc"]},
              {"params": [sh_rest], "lr": LR["sh_rest"]}, {"params": [raw["opacity"]], "lr": LR["opacity"]},
              {"params": [raw["scale"]], "lr": LR["scale"]}, {"params": [raw["rotq"]], "lr": LR["rot"]}]
    opt = torch.optim.Adam(groups, lr=0.0, eps=eps, betas=(0.9, 0.999))
    for g in grads_seq:
        opt.zero_grad()
        act = _activate({**raw, "sh": torch.cat([sh_dc, sh_rest], dim=1)})
        loss = sum((act[k] * torch.tensor(g[k], dtype=torch.float64)).sum() for k in KEYS)
        loss.backward()
        opt.step()
    out = {**{k: raw[k].detach() for k in KEYS if k != "sh"}, "sh": torch.cat([sh_dc, sh_rest], dim=1).detach()}
    return {k: v.numpy() for k, v in out.items()}, {k: v.detach().numpy() for k, v in _activate(out).items()}


def _raw_scene(rng, P):
    return {"pos": rng.normal(0, 1, (P, 3)).astype(np.float32), "scale": rng.normal(-4, 1, (P, 3)).astype(np.float32),
            "rotq": rng.normal(0, 1, (P, 4)).astype(np.float32), "sh": rng.normal(0, 0.3, (P, 48)).astype(np.float32),
            "opacity": rng.normal(0, 2, P).astype(np.float32)}


@pytest.mark.parametrize("aliased", [True, False])
@pytest.mark.parametrize("P", [1, 257, 20011])
def test_adam_step_matches_torch(lcgs, P, aliased):
    """aliased: activated.pos / .sh ARE raw.pos / .sh (identity activation, one array); not aliased: the renderer's
    arrays are separate buffers and the step has to rewrite them too."""
    rng = np.random.default_rng(P)
    raw0 = _raw_scene(rng, P)
    grads_seq = [{k: (rng.normal(0, 1, raw0[k].shape) * 10.0 ** rng.uniform(-4, 0)).astype(np.float32) for k in KEYS}
                 for _ in range(3)]
    eps = 1e-8
    ref_raw, ref_act = _torch_reference(raw0, grads_seq, eps)
    r = lcgs.Renderer(lcgs.Context(0))
    raw = {k: torch.from_numpy(raw0[k]).to(DEV) for k in KEYS}
    m = {k: torch.zeros_like(raw[k]) for k in KEYS}
    v = {k: torch.zeros_like(raw[k]) for k in KEYS}
    act = {k: t.clone() for k, t in _activate(raw).items()}
    if aliased:
        act["pos"], act["sh"] = raw["pos"], raw["sh"]  # raw == activated: one array
    else:
        assert act["pos"].data_ptr() != raw["pos"].data_ptr() and act["sh"].data_ptr() != raw["sh"].data_ptr()
    for step, g in enumerate(grads_seq, 1):
        r.adam_step({k: torch.from_numpy(g[k]).to(DEV) for k in KEYS}, raw, m, v, act, step, LR, eps=eps)
    r.ctx.synchronize()
    for k in KEYS:
        a, b = raw[k].cpu().numpy().astype(np.float64), ref_raw[k]
        assert np.allclose(a, b, rtol=2e-5, atol=2e-6), (k, np.abs(a - b).max())
        a, b = act[k].cpu().numpy().astype(np.float64), ref_act[k]
        assert np.allclose(a, b, rtol=2e-5, atol=2e-6), ("activated " + k, np.abs(a - b).max())
    # the same three steps against the float64 restatement (tests/adam_ref.py, pinned to torch.optim.Adam on the CPU by
    # tests/test_adam_ref.py): raw, activated AND the moments, per array within 3 E32 + 4 u S (the state is the kernels' own after step 1)
    as_torch = lambda d: {k: torch.from_numpy(d[k]) for k in KEYS}
    t64, t32 = [adam_ref.trajectory(as_torch(raw0), [as_torch(g) for g in grads_seq], dt, lr=LR, eps=eps)
                for dt in (torch.float64, torch.float32)]
    for name, pack in zip(adam_ref.ARRAYS, (raw, m, v, act)):
        for k in KEYS:
            diff = float((pack[k].cpu().double() - t64[name][k]).abs().max())
            bound = adam_ref.trajectory_bound(t64[name][k], t32[name][k])
            print(f"[adam] three steps P={P} {name}.{k}: diff / bound {diff / bound:.3f}")
            assert diff <= bound, (name, k, diff, bound)


def test_adam_visible_only_touches_survivors_only(lcgs):
    rng = np.random.default_rng(3)
    P = 4000
    scene = make_scene(rng, P)
    scene["pos"][:1500] += 100.0  # far outside the frustum: culled
    raw = {"pos": scene["pos"], "scale": np.log(scene["scale"]), "rotq": scene["rotq"] * 1.7, "sh": scene["sh"],
           "opacity": np.log(scene["opacity"] / (1 - scene["opacity"]))}
    raw = {k: torch.from_numpy(np.ascontiguousarray(val, dtype=np.float32)).to(DEV) for k, val in raw.items()}
    act = {k: t.clone() for k, t in _activate(raw).items()}
    act["pos"], act["sh"] = raw["pos"], raw["sh"]
    r = lcgs.Renderer(lcgs.Context(0))
    r.bind_scene(*[act[k] for k in KEYS])
    cam = lcgs.get_lookat_cam([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1], width=128, height=96)
    img = torch.zeros(3, 96, 128, device=DEV)
    radii = torch.zeros(P, dtype=torch.int32, device=DEV)
    r.forward(cam, img, radii=radii, keep_state=True)
    g = {k: torch.zeros_like(raw[k]) for k in KEYS}
    r.backward(torch.randn(3, 96, 128, device=DEV), *[g[k] for k in KEYS])
    before = {k: t.clone() for k, t in raw.items()}
    m = {k: torch.zeros_like(raw[k]) for k in KEYS}
    v = {k: torch.zeros_like(raw[k]) for k in KEYS}
    r.adam_step(g, raw, m, v, act, 1, LR, visible_only=True)
    r.ctx.synchronize()
    st = r.frame_stats()
    touched = torch.zeros(P, dtype=torch.bool, device=DEV)
    for k in KEYS:
        touched |= (raw[k] != before[k]).reshape(P, -1).any(dim=1)
    assert not touched[:1500].any()  # culled splats: parameters and moments untouched
    assert all((m[k][:1500] == 0).all() and (v[k][:1500] == 0).all() for k in KEYS)
    assert 0 < int(touched.sum()) <= st["num_visible"]
    # survivors with a non-zero gradient moved, exactly as in the dense step
    raw_d = {k: before[k].clone() for k in KEYS}
    act_d = {k: t.clone() for k, t in _activate(raw_d).items()}
    act_d["pos"], act_d["sh"] = raw_d["pos"], raw_d["sh"]
    md = {k: torch.zeros_like(raw[k]) for k in KEYS}
    vd = {k: torch.zeros_like(raw[k]) for k in KEYS}
    r.adam_step(g, raw_d, md, vd, act_d, 1, LR, visible_only=False)
    r.ctx.synchronize()
    vis = (radii > 0)
    for k in KEYS:
        assert torch.equal(raw[k][vis], raw_d[k][vis]), k


def test_compact_gradient_rows_and_their_optimiser_step(lcgs, oracle):
    """lcgs_render_backward_compact: row r = the r-th on-screen splat (ascending index, lcgs_visible_rows), equal to
    that splat's row of the dense gradients, nothing else written; lcgs_adam_step(visible_only = 2) on those rows equals
    the on-screen-only step on the dense gradients bit for bit."""
    rng = np.random.default_rng(5)
    P = 30000
    scene = make_scene(rng, P, log_scale=(-3.9, 0.6))
    scene["pos"][5000:9000] += 100.0  # culled block in the middle of the index range
    raw = {"pos": scene["pos"], "scale": np.log(scene["scale"]), "rotq": scene["rotq"] * 1.3, "sh": scene["sh"],
           "opacity": np.log(scene["opacity"] / (1 - scene["opacity"]))}
    raw = {k: torch.from_numpy(np.ascontiguousarray(val, dtype=np.float32)).to(DEV) for k, val in raw.items()}
    act = {k: t.clone() for k, t in _activate(raw).items()}
    act["pos"], act["sh"] = raw["pos"], raw["sh"]
    r = lcgs.Renderer(lcgs.Context(0))
    r.bind_scene(*[act[k] for k in KEYS])
    W, H = 320, 200
    cam = lcgs.get_lookat_cam([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1], width=W, height=H)
    img = torch.zeros(3, H, W, device=DEV)
    dL = torch.randn(3, H, W, device=DEV)
    r.forward(cam, img, keep_state=True, sync=True)
    dense = {k: torch.full_like(raw[k], 7.0) for k in KEYS}
    r.backward(dL, *[dense[k] for k in KEYS])
    rows = r.visible_rows().long()
    V = r.frame_stats()["num_visible"]
    assert rows.numel() == V and 0 < V < P
    assert (rows[1:] > rows[:-1]).all()  # ascending splat index
    assert not ((rows >= 5000) & (rows < 9000)).any()
    comp = {k: torch.full_like(raw[k], 7.0) for k in KEYS}  # P rows allocated, V of them used
    r.backward(dL, *[comp[k] for k in KEYS], compact=True)  # a second backward of the same frame
    r.ctx.synchronize()
    for k in KEYS:
        c, d = comp[k].reshape(P, -1), dense[k].reshape(P, -1)
        # (pixel-to-splat sums are float atomics: two backward passes of one frame differ in the last bits of the 2-D
        # gradients, which the geometry Jacobians amplify on ill-conditioned splats -- compare in the norm)
        err = (c[:V].double() - d[rows].double()).norm() / d[rows].double().norm()
        assert err <= 1e-4, (k, float(err))
        assert (c[V:] == 7.0).all(), k  # rows beyond the on-screen count are not touched
        off = torch.ones(P, dtype=torch.bool, device=DEV)
        off[rows] = False
        assert (d[off] == 0).all(), k  # the dense variant: exact zeros elsewhere
    # both against the f64 oracle row by row: compact row r is splat rows[r]'s row
    bound = gradient_row_bound({k: act[k].cpu().numpy() for k in KEYS}, oracle.lookat([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1],
                                                                                       width=W, height=H), dL.cpu().numpy())
    check_gradient_rows(dense, None, None, None, bound=bound, tag="dense")
    check_gradient_rows({k: comp[k].reshape(P, -1)[:V] for k in KEYS}, None, None, None, bound=bound,
                        rows=rows.cpu().numpy(), tag="compact rows")
    # optimiser: compact rows (mode 2) vs the same gradients scattered to their splats (mode 1)
    scattered = {k: torch.zeros_like(raw[k]) for k in KEYS}
    for k in KEYS:
        scattered[k].reshape(P, -1)[rows] = comp[k].reshape(P, -1)[:V]
    state = []
    for compact in (False, True):
        rw = {k: t.clone() for k, t in raw.items()}
        ac = {k: t.clone() for k, t in _activate(rw).items()}
        ac["pos"], ac["sh"] = rw["pos"], rw["sh"]
        m = {k: torch.zeros_like(rw[k]) for k in KEYS}
        v = {k: torch.zeros_like(rw[k]) for k in KEYS}
        r.adam_step(comp if compact else scattered, rw, m, v, ac, 1, LR, visible_only=True, compact_grads=compact)
        r.ctx.synchronize()
        state.append((rw, m, v, ac))
    for a, b in zip(state[0], state[1]):
        for k in KEYS:
            assert torch.equal(a[k], b[k]), k
    assert not torch.equal(state[0][0]["sh"], raw["sh"])  # and something moved
    with pytest.raises(ValueError):
        r.adam_step(comp, raw, m, v, act, 1, LR, visible_only=False, compact_grads=True)


def test_autograd_binding_matches_oracle_backward(lcgs, oracle):
    rng = np.random.default_rng(8)
    scene = make_scene(rng, 3000, log_scale=(-3.6, 0.7))
    W, H = 128, 96
    pose = ([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1])
    cam = lcgs.get_lookat_cam(*pose, width=W, height=H)
    t = {k: torch.from_numpy(scene[k]).to(DEV).requires_grad_(True) for k in KEYS}
    r = lcgs.Renderer(lcgs.Context(0))
    img = lcgs.render_autograd(r, cam, *[t[k] for k in KEYS], bg=(0.1, 0.2, 0.3))
    dL = torch.from_numpy(np.random.default_rng(0).normal(size=(3, H, W)).astype(np.float32)).to(DEV)
    (img * dL).sum().backward()
    ref = oracle.render_backward_full(scene, oracle.lookat(*pose, width=W, height=H), dL.cpu().numpy(), bg=(0.1, 0.2, 0.3))
    for k in KEYS:
        a, b = t[k].grad.cpu().numpy().astype(np.float64), ref[k].astype(np.float64).reshape(t[k].shape)
        assert np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30) <= 1e-3, k
    check_gradient_rows({k: t[k].grad for k in KEYS}, scene, oracle.lookat(*pose, width=W, height=H), dL.cpu().numpy(),
                        bg=(0.1, 0.2, 0.3), ref32=ref, tag="autograd")


def test_autograd_multi_view_loss_and_interleaved_use(lcgs, oracle):
    """Two render_autograd frames of ONE renderer alive at once (a two-view loss), plus an unrelated forward in between:
    each view's backward must differentiate its own frame (the binding re-renders a view whose state was replaced)."""
    rng = np.random.default_rng(18)
    scene = make_scene(rng, 3000, log_scale=(-3.6, 0.7))
    W, H = 128, 96
    poses = [([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1]), ([2.5, 1.5, 1.0], [0, 0, 0.5], [0, 0, 1])]
    cams = [lcgs.get_lookat_cam(*p, width=W, height=H) for p in poses]
    t = {k: torch.from_numpy(scene[k]).to(DEV).requires_grad_(True) for k in KEYS}
    r = lcgs.Renderer(lcgs.Context(0))
    imgs = [lcgs.render_autograd(r, c, *[t[k] for k in KEYS], bg=(0.1, 0.2, 0.3)) for c in cams]
    r.forward(cams[0], torch.zeros(3, H, W, device=DEV), keep_state=False)  # somebody else uses the renderer
    dLs = [torch.from_numpy(np.random.default_rng(i).normal(size=(3, H, W)).astype(np.float32)).to(DEV) for i in range(2)]
    sum((img * dL).sum() for img, dL in zip(imgs, dLs)).backward()
    refs = [oracle.render_backward_full(scene, oracle.lookat(*p, width=W, height=H), dL.cpu().numpy(), bg=(0.1, 0.2, 0.3))
            for p, dL in zip(poses, dLs)]
    for k in KEYS:
        a = t[k].grad.cpu().numpy().astype(np.float64)
        b = sum(ref[k].astype(np.float64).reshape(t[k].shape) for ref in refs)
        assert np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30) <= 1e-3, k
    # per row: the bound of a sum of views is the sum of the views' bounds
    bounds = [gradient_row_bound(scene, oracle.lookat(*p, width=W, height=H), dL.cpu().numpy(), bg=(0.1, 0.2, 0.3), ref32=ref)
              for p, dL, ref in zip(poses, dLs, refs)]
    check_gradient_rows({k: t[k].grad for k in KEYS}, None, None, None, tag="autograd, two views",
                        bound=({k: bounds[0][0][k] + bounds[1][0][k] for k in KEYS},
                               {k: bounds[0][1][k].astype(np.float64) + bounds[1][1][k] for k in KEYS}))


def test_adam_step_argument_checks(lcgs):
    r = lcgs.Renderer(lcgs.Context(0))
    z = {k: torch.zeros(s, device=DEV) for k, s in zip(KEYS, ((4, 3), (4, 3), (4, 4), (4, 48), (4,)))}
    with pytest.raises(lcgs.LcgsError):
        r.adam_step(z, z, z, z, z, 0, LR)  # step counts from 1
    with pytest.raises(lcgs.LcgsError):
        r.adam_step(z, z, z, z, z, 1, LR, visible_only=True)  # no forward frame in this context


def test_fit_views_equals_the_views_one_after_the_other(lcgs):
    """lcgs_fit_views (views alternating between the context and its sibling, a forward beside the previous backward) gives
    what forward -> L2 loss -> backward(_accumulate) per view give: the same losses and gradient sums up to the order of
    float additions."""
    import torch

    from bench import view_pose
    from conftest import make_scene
    from gpu_util import DEV, upload_scene

    rng = np.random.default_rng(77)
    P, W, H = 40000, 320, 240
    scene = make_scene(rng, P, spread=1.5, log_scale=(-3.6, 0.6))
    d = upload_scene(scene)
    KEYS = ("pos", "scale", "rotq", "sh", "opacity")
    shapes = {"pos": (P, 3), "scale": (P, 3), "rotq": (P, 4), "sh": (P, 48), "opacity": (P,)}
    for n_views in (1, 2, 3, 4):
        cams = [lcgs.get_lookat_cam(*view_pose(k), width=W, height=H) for k in range(n_views)]
        targets = [torch.rand(3, H, W, device=DEV) for _ in range(n_views)]
        # reference: one view after the other on a single context
        r = lcgs.Renderer(lcgs.Context(0))
        r.bind_scene(*[d[k] for k in KEYS])
        want = {k: torch.full(shapes[k], 7.0, device=DEV) for k in KEYS}
        want_loss = torch.zeros(n_views, device=DEV)
        img, dL = torch.zeros(3, H, W, device=DEV), torch.zeros(3, H, W, device=DEV)
        for j, cam in enumerate(cams):
            r.forward(cam, img, keep_state=True, sync=False)
            r.l2_loss_backward(img, targets[j], dL, want_loss[j:j + 1])
            r.backward(dL, *[want[k] for k in KEYS], accumulate=j > 0)
        r.ctx.synchronize()
        # the batch call, twice on one context (the second step starts from stale arrays and a warm sibling)
        r2 = lcgs.Renderer(lcgs.Context(0))
        r2.bind_scene(*[d[k] for k in KEYS])
        for rep in range(2):
            got = {k: torch.full(shapes[k], -3.0, device=DEV) for k in KEYS}
            got_loss = torch.full((n_views,), -1.0, device=DEV)
            torch.cuda.synchronize()
            r2.fit_views(cams, targets, *[got[k] for k in KEYS], got_loss)
            r2.ctx.synchronize()
            assert torch.allclose(got_loss, want_loss, rtol=1e-5, atol=0.0), (n_views, rep)  # (an atomic float sum)
            for k in KEYS:
                num = (got[k] - want[k]).double().norm().item()
                den = want[k].double().norm().item()
                assert num <= 2e-4 * den + 1e-12, (n_views, rep, k, num, den)
                assert torch.equal(got[k] == 0, want[k] == 0), (n_views, rep, k)


@pytest.mark.parametrize("separate_act", [False, True])
def test_backward_with_the_optimiser_folded_in_equals_the_two_calls(lcgs, separate_act):
    """lcgs_render_backward_adam: the on-screen-only Adam update applied inside the kernel that forms the per-splat
    gradients (no gradient arrays) against lcgs_render_backward_compact + lcgs_adam_step(visible_only = 2).  The same
    arithmetic in the same order -- but the pixel-to-splat sums behind both are float atomics, so two backward passes of one
    frame differ in the last bits and Adam's first step turns the sign of a near-zero gradient into +-lr: almost every
    element must agree to a small fraction of lr, none may differ by more than the 2 lr of a sign flip, and the rows of
    splats that did not reach the screen must be untouched, bit for bit."""
    rng = np.random.default_rng(6)
    P = 30000
    scene = make_scene(rng, P, log_scale=(-3.9, 0.6))
    scene["pos"][5000:9000] += 100.0  # culled block in the middle of the index range
    raw0 = {"pos": scene["pos"], "scale": np.log(scene["scale"]), "rotq": scene["rotq"] * 1.3, "sh": scene["sh"],
            "opacity": np.log(scene["opacity"] / (1 - scene["opacity"]))}
    raw0 = {k: torch.from_numpy(np.ascontiguousarray(val, dtype=np.float32)).to(DEV) for k, val in raw0.items()}
    W, H = 320, 200
    cam = lcgs.get_lookat_cam([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1], width=W, height=H)
    dL = torch.randn(3, H, W, device=DEV)
    lr_of = {"pos": LR["pos"], "scale": LR["scale"], "rotq": LR["rot"], "sh": LR["sh_dc"], "opacity": LR["opacity"]}
    out = {}
    for fused in (False, True):
        raw = {k: t.clone() for k, t in raw0.items()}
        act = {k: t.clone() for k, t in _activate(raw).items()}
        if not separate_act:
            act["pos"], act["sh"] = raw["pos"], raw["sh"]  # identity activations: one array
        m = {k: torch.zeros_like(raw[k]) for k in KEYS}
        v = {k: torch.zeros_like(raw[k]) for k in KEYS}
        r = lcgs.Renderer(lcgs.Context(0))
        r.bind_scene(*[act[k] for k in KEYS])
        img = torch.zeros(3, H, W, device=DEV)
        r.forward(cam, img, keep_state=True, sync=False)
        if fused:
            r.backward_adam(dL, raw, m, v, act, 1, LR, eps=1e-8)
        else:
            g = {k: torch.zeros_like(raw[k]) for k in KEYS}
            r.backward(dL, *[g[k] for k in KEYS], compact=True)
            r.adam_step(g, raw, m, v, act, 1, LR, eps=1e-8, visible_only=True, compact_grads=True)
        r.ctx.synchronize()
        rows = r.visible_rows().long()
        out[fused] = (raw, m, v, act, rows)
        if fused:  # a second step on the moved scene: still finite, still training (the frame reads what the step wrote)
            r.forward(cam, img, keep_state=True, sync=False)
            before = raw["opacity"].clone()
            raw2 = {k: t.clone() for k, t in raw.items()}
            r.backward_adam(dL, raw, m, v, act, 2, LR, eps=1e-8)
            r.ctx.synchronize()
            assert all(torch.isfinite(raw[k]).all() for k in KEYS) and not torch.equal(raw["opacity"], before)
            out[fused] = (raw2, m, v, act, rows)
    (raw_a, m_a, v_a, act_a, rows), (raw_b, m_b, v_b, act_b, rows_b) = out[False], out[True]
    assert torch.equal(rows, rows_b) and 0 < rows.numel() < P
    off = torch.ones(P, dtype=torch.bool, device=DEV)
    off[rows] = False
    for k in KEYS:
        assert not torch.equal(raw_b[k][rows], raw0[k][rows]), k  # it trained ...
        assert torch.equal(raw_b[k][off], raw0[k][off]), k  # ... and only the on-screen rows
        diff = (raw_b[k] - raw_a[k]).abs()
        assert float(diff.max()) <= 2.02 * lr_of[k], (k, float(diff.max()))
        assert float((diff > 0.05 * lr_of[k]).float().mean()) < 0.01, k


def test_backward_adam_on_other_sh_degrees_runs_the_two_calls(lcgs):
    """degree < 3 (no kept colour Jacobian): lcgs_render_backward_adam falls back to compact rows + lcgs_adam_step inside
    the library -- same entry point, same result as the caller doing the two calls."""
    rng = np.random.default_rng(8)
    P = 8000
    scene = make_scene(rng, P, log_scale=(-3.9, 0.6))
    lib = lcgs.load_library()
    # (the Python mirror binds degree-3 scenes; this check goes through the C ABI directly for degree 1)
    import ctypes as C

    deg, feat = 1, 12
    raw = {"pos": torch.from_numpy(scene["pos"]).to(DEV), "scale": torch.from_numpy(np.log(scene["scale"])).to(DEV),
           "rotq": torch.from_numpy(scene["rotq"] * 1.3).to(DEV), "sh": torch.from_numpy(scene["sh"][:, :feat].copy()).to(DEV),
           "opacity": torch.from_numpy(np.log(scene["opacity"] / (1 - scene["opacity"]))).to(DEV)}
    act = {"pos": raw["pos"], "scale": torch.exp(raw["scale"]), "rotq": raw["rotq"] / raw["rotq"].norm(dim=1, keepdim=True),
           "sh": raw["sh"], "opacity": torch.sigmoid(raw["opacity"])}
    before = raw["opacity"].clone()
    ctx = lcgs.Context(0)
    P_ = C.c_int(P)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert lib.lcgs_scene_bind(ctx._h, P_, C.c_int(deg), ptr(act["pos"]), ptr(act["scale"]), ptr(act["rotq"]), ptr(act["sh"]),
                               ptr(act["opacity"])) == 0
    cam = lcgs.get_lookat_cam([-3, -0.5, 2.3], [0, 0, 0.5], [0, 0, 1], width=160, height=120)
    img = torch.zeros(3, 120, 160, device=DEV)
    n = C.c_int(0)
    bg = (C.c_float * 3)(0, 0, 0)
    assert lib.lcgs_render_forward(ctx._h, C.byref(cam), bg, C.c_float(1.0), ptr(img), None, 1, C.byref(n)) == 0 and n.value > 0
    m = {k: torch.zeros_like(raw[k]) for k in KEYS}
    v = {k: torch.zeros_like(raw[k]) for k in KEYS}
    cfg = lcgs.api._AdamConfig(LR["pos"], LR["sh_dc"], LR["sh_rest"], LR["opacity"], LR["scale"], LR["rot"], 0.9, 0.999, 1e-8, 1, 2)
    packs = [lcgs.api._Params(*[ptr(d_[k]) for k in KEYS]) for d_ in (raw, m, v, act)]
    dL = torch.randn(3, 120, 160, device=DEV)
    st = lib.lcgs_render_backward_adam(ctx._h, ptr(dL), P_, C.c_int(deg), C.byref(cfg), *[C.byref(p) for p in packs])
    assert st == 0, lib.lcgs_last_error()
    ctx.synchronize()
    assert not torch.equal(raw["opacity"], before) and torch.isfinite(raw["opacity"]).all()
    assert float((m["sh"] != 0).float().mean()) > 0.01


def test_fused_step_equals_the_two_calls_bit_for_bit_on_a_lattice_frame(lcgs, oracle):
    """lcgs_render_backward_adam against lcgs_render_backward_compact + lcgs_adam_step(visible_only = 2), torch.equal on all
    five arrays of raw / m / v / activated, on a frame whose 2-D gradients are deterministic: 260 small splats (V = 260: two
    workgroups of the per-splat kernels, the last wave with four valid lanes), each at the centre of its own 8 x 8-pixel
    quadrant of a 320 x 200 frame with its pixel rectangle inside that quadrant.  A quadrant is one wave of the
    render-backward, so every splat's 2-D gradient row is ONE wave's sums added once onto zero (one LDS add, one global add
    per tile): no order of float atomics to differ in.  The reference's rect clamp leaves the last tile column and row
    empty, so the lattice of every second quadrant in x and y has 19 x 12 = 228 usable sites; the other 32 splats sit on
    the odd / odd quadrants of the first tiles (their own quadrant each, 11 px from the nearest lattice centre).  Those 32
    share a 16 x 16 tile with lattice splats, and so do the lattice splats with them.  For these the argument rests on the
    tile's other three waves contributing EXACT zeros: a foreign wave either skips the entry (its strip bit is clear) or
    walks it with every lane below alpha = 1/255 (no pixel of a foreign quadrant lies inside the splat's reach, asserted
    below), and such a lane carries alpha 0 and terms that are all 0.0; x + 0.0 == x in whatever order the LDS adds land.
    40 more splats are culled: rows that did not reach the screen must be untouched."""
    W, H, depth, n_off = 320, 200, 4.0, 40
    pose = ([0.0, -4.0, 0.5], [0.0, 0.0, 0.5], [0.0, 0.0, 1.0])
    ocam = oracle.lookat(*pose, width=W, height=H)
    c, front, right, up = (np.array(v[:], dtype=np.float64) for v in (ocam.position, ocam.front, ocam.right, ocam.up))

    def project(pos, scale, rotq):  # the oracle's pixel means, radii and tile counts
        m2, z, cov = oracle.project(pos, scale, rotq, ocam)
        means, _, tiles, radii = oracle.allocate_tiles(W, H, z, m2, cov)
        return means.astype(np.float64), radii, tiles

    # at a fixed depth the pixel mean is an affine function of the in-plane coordinates: fitted through three probes
    probes = np.stack([c + depth * front, c + depth * front + right, c + depth * front + up]).astype(np.float32)
    mp, _, _ = project(probes, np.full((3, 3), 1e-3, np.float32), np.tile(np.float32([1, 0, 0, 0]), (3, 1)))
    A = np.stack([mp[1] - mp[0], mp[2] - mp[0]], axis=1)
    even = [(qx, qy) for qy in range(0, 24, 2) for qx in range(0, 38, 2)]
    quads = np.array(even + [(qx, qy) for qy in (1, 3) for qx in range(1, 33, 2)])  # 228 + 32
    n_on = len(quads)
    assert n_on == 260 and len({tuple(q) for q in quads}) == n_on
    ab = np.linalg.solve(A, (8.0 * quads + 3.5 - mp[0]).T).T
    rng = np.random.default_rng(11)
    P = n_on + n_off
    on = np.ones(P, dtype=bool)
    on[100:100 + n_off] = False  # the culled block, in the middle of the index range
    scene = make_scene(rng, P)
    scene["pos"][on] = (c + depth * front + ab[:, :1] * right + ab[:, 1:] * up).astype(np.float32)
    scene["pos"][~on] += 100.0
    scene["scale"] = (rng.uniform(0.25, 0.4, (P, 3)) / np.sqrt(abs(np.linalg.det(A)))).astype(np.float32)  # 0.25 .. 0.4 px
    scene["opacity"] = rng.uniform(0.2, 0.95, P).astype(np.float32)
    # the precondition, on the CPU: every on-screen splat claims one tile and its rect [mean - r, mean + r] lies inside the
    # pixels 8 q .. 8 q + 7 of its quadrant.  (r >= 3 sigma and alpha >= 1/255 ends within 3.33 sigma: it then reaches no
    # pixel of another quadrant, whose nearest centre is 4.5 px from the mean.)
    means, radii, tiles = project(scene["pos"], scene["scale"], scene["rotq"])
    assert (tiles[on] == 1).all() and (radii[on] > 0).all() and (tiles[~on] == 0).all()
    assert (np.floor(means[on] - radii[on, None]) >= 8 * quads).all() and (np.ceil(means[on] + radii[on, None]) <= 8 * quads + 7).all()

    raw0 = {"pos": scene["pos"], "scale": np.log(scene["scale"]), "rotq": scene["rotq"] * 1.3, "sh": scene["sh"],
            "opacity": np.log(scene["opacity"] / (1 - scene["opacity"]))}
    raw0 = {k: torch.from_numpy(np.ascontiguousarray(val, dtype=np.float32)).to(DEV) for k, val in raw0.items()}
    cam = lcgs.get_lookat_cam(*pose, width=W, height=H)
    dL = torch.from_numpy(rng.normal(size=(3, H, W)).astype(np.float32)).to(DEV)
    off = torch.from_numpy(~on).to(DEV)
    for separate_act in (False, True):
        out = {}
        for fused in (False, True):
            raw = {k: t.clone() for k, t in raw0.items()}
            act = {k: t.clone() for k, t in _activate(raw).items()}
            if not separate_act:
                act["pos"], act["sh"] = raw["pos"], raw["sh"]  # identity activations: one array
            m = {k: torch.zeros_like(raw[k]) for k in KEYS}
            v = {k: torch.zeros_like(raw[k]) for k in KEYS}
            r = lcgs.Renderer(lcgs.Context(0))
            r.bind_scene(*[act[k] for k in KEYS])
            r.forward(cam, torch.zeros(3, H, W, device=DEV), keep_state=True, sync=False)
            if fused:
                r.backward_adam(dL, raw, m, v, act, 1, LR, eps=1e-8)
            else:
                g, g2 = [{k: torch.zeros_like(raw[k]) for k in KEYS} for _ in range(2)]
                r.backward(dL, *[g[k] for k in KEYS], compact=True)
                r.backward(dL, *[g2[k] for k in KEYS], compact=True)
                r.ctx.synchronize()
                for k in KEYS:  # the premise: two backward passes of this frame give the same bits
                    assert torch.equal(g[k], g2[k]), ("two compact backward passes differ", k)
                    assert g[k].reshape(P, -1)[:n_on].abs().sum() > 0, k
                r.adam_step(g, raw, m, v, act, 1, LR, eps=1e-8, visible_only=True, compact_grads=True)
            r.ctx.synchronize()
            assert r.frame_stats()["num_visible"] == n_on
            assert torch.equal(r.visible_rows().long(), torch.nonzero(~off).ravel())
            out[fused] = {"raw": raw, "m": m, "v": v, "act": act}
        for name in ("raw", "m", "v", "act"):
            for k in KEYS:
                a, b = out[False][name][k], out[True][name][k]
                assert torch.equal(a, b), (separate_act, name, k, int((a != b).sum()))
        for k in KEYS:
            got = out[True]
            assert not torch.equal(got["raw"][k][~off], raw0[k][~off]), k  # it trained ...
            assert torch.equal(got["raw"][k][off], raw0[k][off]), k  # ... and only the on-screen rows
            assert (got["m"][k][off] == 0).all() and (got["v"][k][off] == 0).all(), k
            assert torch.equal(got["act"][k][off], _activate(raw0)[k][off]), k
