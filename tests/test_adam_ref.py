"""The yardstick of the optimiser step pinned without a GPU (tests/adam_ref.py): step64 is torch.optim.Adam behind autograd,
step32 stays inside the first-order bound on every input class the GPU tests use (they assert twice that bound), the bound flags
what it should, and the row-list modes touch the rows they are given."""
import pytest
import torch

import adam_ref as R

P_BOUND = 20011


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def _torch_adam(raw0, grads_seq, s_of_step, sh_floats):
    """torch.optim.Adam in float64 on the raw parameters, gradients w.r.t. the activated values pushed through autograd (the
    construction of test_gpu_train._torch_reference), fed the binary32 scalars -> raw, m, v, activated after the last step"""
    s = s_of_step(1)
    raw = {k: t.double().clone().requires_grad_(True) for k, t in raw0.items()}
    sh_dc = raw0["sh"].double()[:, :3].clone().requires_grad_(True)
    sh_rest = raw0["sh"].double()[:, 3:].clone().requires_grad_(True)
    lr = s["lr"]
    groups = [{"params": [raw["pos"]], "lr": lr["pos"]}, {"params": [sh_dc], "lr": lr["sh_dc"]},
              {"params": [raw["opacity"]], "lr": lr["opacity"]}, {"params": [raw["scale"]], "lr": lr["scale"]},
              {"params": [raw["rotq"]], "lr": lr["rot"]}]
    if sh_floats > 3:
        groups.append({"params": [sh_rest], "lr": lr["sh_rest"]})
    opt = torch.optim.Adam(groups, lr=0.0, eps=s["eps"], betas=(s["b1"], s["b2"]))
    sh = lambda: torch.cat([sh_dc, sh_rest], dim=1)
    for g in grads_seq:
        opt.zero_grad()
        act = R.activate64({**raw, "sh": sh()})
        sum((act[k] * g[k].double()).sum() for k in R.KEYS).backward()
        opt.step()
    out = {**{k: raw[k].detach() for k in R.KEYS if k != "sh"}, "sh": sh().detach()}
    st = lambda p, name: opt.state[p][name]
    mom = {name: {**{k: st(raw[k], name) for k in R.KEYS if k != "sh"},
                  "sh": torch.cat([st(sh_dc, name)] + ([st(sh_rest, name)] if sh_floats > 3 else []), dim=1)}
           for name in ("exp_avg", "exp_avg_sq")}
    return {"raw": out, "m": mom["exp_avg"], "v": mom["exp_avg_sq"], "act": R.activate64(out)}


def _start(P, sh_floats, seed):
    gen = torch.Generator().manual_seed(seed)
    n = lambda shape, mu, sd: (mu + sd * torch.randn(shape, generator=gen, dtype=torch.float64)).float()
    shp = R.shapes(P, sh_floats)
    raw0 = {"pos": n(shp["pos"], 0, 1), "scale": n(shp["scale"], -4, 1), "rotq": n(shp["rotq"], 0, 1), "sh": n(shp["sh"], 0, 0.3),
            "opacity": n(shp["opacity"], 0, 2)}
    grads = [{k: (n(shp[k], 0, 1).double() * 10.0 ** (-4.0 * torch.rand((), generator=gen, dtype=torch.float64))).float()
              for k in R.KEYS} for _ in range(5)]
    return raw0, grads


@pytest.mark.parametrize("eps", R.EPSES)
@pytest.mark.parametrize("degree", [0, 3])
def test_step64_is_torch_adam_behind_autograd(degree, eps):
    F = 3 * (degree + 1) ** 2
    raw0, grads = _start(61, F, 10 * degree + 1)
    want = _torch_adam(raw0, grads, lambda t: R.scalars(t, eps=eps), F)
    got = R.trajectory(raw0, grads, torch.float64, eps=eps)
    for a in R.ARRAYS:
        for k in R.KEYS:
            assert _rel(got[a][k], want[a][k]) <= 1e-12, (a, k, _rel(got[a][k], want[a][k]))


@pytest.mark.parametrize("step", R.STEPS)
@pytest.mark.parametrize("cls", R.CLASSES)
def test_step32_stays_inside_the_first_order_bound(cls, step):
    """half of what the GPU tests assert; per attribute and array, both eps, degree 0 and 3"""
    worst = {}
    for eps in R.EPSES:
        if cls == "saturation" and eps != 1e-15:
            continue
        s = R.scalars(step, eps=eps)
        for F in (3, 48):
            inp = R.make_inputs(cls, P_BOUND, F, 1000 * step + F, s)
            res = R.check(R.step32(*inp, s), *inp, s, factor=1.0)
            assert not R.failures(res), (eps, F, R.failures(res))
            for (a, k), (ratio, _) in res.items():
                worst[(a, k)] = max(worst.get((a, k), 0.0), ratio)
    print(f"[adam_ref] {cls} step {step}: step32 / first-order bound  " + "  ".join(
        f"{a} " + "/".join(f"{worst[(a, k)]:.3f}" for k in R.KEYS) for a in R.ARRAYS))


def _general(P=257, F=48, step=10, eps=1e-8, seed=5):
    s = R.scalars(step, eps=eps)
    return R.make_inputs("general", P, F, seed, s), s


def test_one_element_three_bounds_away_is_flagged():
    inp, s = _general()
    ref, bnd = R.step64(*inp, s), R.bound(*inp, s)
    clean = {a: {k: ref[a][k].clone() for k in R.KEYS} for a in R.ARRAYS}
    assert not R.failures(R.check(clean, *inp, s))
    for a in R.ARRAYS:
        for k in R.KEYS:
            i = ref[a][k].numel() // 2
            b = bnd[a][k].reshape(-1)[i]
            assert 0 < float(b) < float("inf")
            moved = {x: dict(clean[x]) for x in R.ARRAYS}
            moved[a][k] = clean[a][k].clone()
            moved[a][k].view(-1)[i] += 3.0 * b
            bad = R.failures(R.check(moved, *inp, s))
            assert list(bad) == [(a, k)] and bad[(a, k)][1] == 1, (a, k, bad)


@pytest.mark.parametrize("mutant", [1, 2, 3, 4, 5, 6, 7])
def test_the_bound_flags_every_kernel_mutant(mutant):
    """the seven one-line mutants of docs/TESTS.md applied to step32 (7, the grid-stride loop cut to one pass: the rows behind
    the first pass keep their input), at the asserted 2 x bound"""
    inp, s = _general()
    assert not R.failures(R.check(R.step32(*inp, s), *inp, s))
    got = R.step32(*inp, s, mutant=0 if mutant == 7 else mutant)
    if mutant == 7:
        start = dict(zip(R.ARRAYS, inp[1:]))
        for a in R.ARRAYS:
            for k in R.KEYS:
                got[a][k][200:] = start[a][k][200:]
    bad = R.failures(R.check(got, *inp, s))
    assert bad, mutant
    hit = {1: ("raw", "pos"), 2: ("raw", "pos"), 3: ("m", "pos"), 4: ("v", "pos"), 5: ("raw", "sh"), 6: ("m", "opacity"),
           7: ("m", "rotq")}[mutant]
    assert hit in bad, (mutant, sorted(bad))
    if mutant == 5:  # column 3 alone, on raw and activated
        assert set(bad) == {("raw", "sh"), ("act", "sh")}
        clean = R.step32(*inp, s)
        differs = (got["raw"]["sh"] != clean["raw"]["sh"]).any(dim=0)
        assert bool(differs[3]) and int(differs.sum()) == 1


def test_row_list_modes_touch_the_listed_rows_only():
    inp, s = _general(P=9, F=12)
    g, raw, m, v, act = inp
    rows = torch.tensor([7, 2, 5])
    dense = R.step64(*inp, s)
    for fn, dtype in ((R.step64, torch.float64), (R.step32, torch.float32)):
        one = fn(*inp, s, rows=rows)
        compact_g = {k: torch.full_like(g[k], 7.0) for k in R.KEYS}
        for k in R.KEYS:
            compact_g[k][:3] = g[k][rows]
        two = fn(compact_g, raw, m, v, act, s, rows=rows, compact=True)
        start = dict(zip(R.ARRAYS, (raw, m, v, act)))
        off = torch.ones(9, dtype=torch.bool)
        off[rows] = False
        for a in R.ARRAYS:
            for k in R.KEYS:
                assert one[a][k].dtype == dtype and torch.equal(one[a][k], two[a][k])  # compact row r is splat rows[r]'s
                assert torch.equal(one[a][k][off], start[a][k][off].to(dtype)), (a, k)  # untouched, bit for bit
                if dtype == torch.float64:
                    assert torch.equal(one[a][k][rows], dense[a][k][rows]), (a, k)
                assert not torch.equal(one[a][k][rows], start[a][k][rows].to(dtype)), (a, k)
    bnd = R.bound(*inp, s, rows=rows)
    assert all(bool((bnd[a][k][off] == 0).all()) and bool((bnd[a][k][rows] > 0).all()) for a in R.ARRAYS for k in R.KEYS)
