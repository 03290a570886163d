"""`-m "not gpu"`: every `*_premise` of tests/test_gpu_owner_rows.py on the CPU -- a premise needs only the oracle, so what each
scene claims about its frames (which rows of which span are on screen, which views are empty, that a padded segment is
longer than its rows) is checked without a GPU, and a failing GPU case cannot be blamed on its frame."""
import pytest

import test_gpu_owner_rows as T

COVERED = {"halves_premise", "boundary_premise", "ranks_premise", "padding_premise", "clipped_premise"}


def _run(fn, *args):
    assert fn.__name__ in COVERED
    return fn(*args)


def test_halves(oracle):
    for name in T.HALVES_POSES:
        v = _run(T.halves_premise, oracle, name)
        assert (v.W, v.H, v.P) == (200, 150, 4001)
    for deg in (0, 1, 2):
        _run(T.halves_premise, oracle, "near", deg)
    for spans in T.SPANS.values():  # the spans tile [53, 3864)
        assert spans[0][0] == T.HEAD and spans[-1][0] + spans[-1][1] == T.END
        assert all(a[0] + a[1] == b[0] for a, b in zip(spans, spans[1:]))


@pytest.mark.parametrize("V", T.BOUNDARY_V)
def test_boundary(oracle, V):
    v = _run(T.boundary_premise, oracle, V)
    a, b = T.INNER[0], T.INNER[0] + T.INNER[1]
    assert int(v.on[a:b].sum()) == V == int(v.hit[a:b].sum())


@pytest.mark.parametrize("world", [2, 3])
def test_ranks(oracle, world):
    views = _run(T.ranks_premise, oracle, world)
    assert len(views) == world and views[0].P == {2: 6001, 3: 9001}[world]


def test_padding(oracle):
    assert len(_run(T.padding_premise, oracle)) == 3


def test_clipped(oracle):
    away, at = _run(T.clipped_premise, oracle)
    assert len(away) == len(at) == 3 and at[0].P == 9001


def test_every_premise_of_the_file_is_covered_here():
    names = {n for n in dir(T) if n.endswith("_premise") and callable(getattr(T, n))}
    assert names == COVERED, names ^ COVERED
