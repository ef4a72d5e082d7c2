"""The host-or-device routing of binding.Model's calls (Model._route): update, change_rows, separate_triangles,
separate_cliques, inactive_rows, round and bound take NumPy arrays (host route) or CUDA float64 tensors (device route).  A
mixture of the two, and an input of the wrong length on either route, is a ValueError raised in Python before a pointer is
handed to the library -- so the model's counters do not move and its next solve returns the bits of the one before.  The two
separations take ONE vector and have nothing to mix: for them the two routes return equal outputs.

The model is the smallest with every ingredient: one PSD cone of side 6 (n = 21), diag X = 1 as the p = 6 equality rows, and
m = 2 inequality rows (two triangle inequalities of the nodes 0, 1, 2)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P

import model_rows_cases as R

pytestmark = pytest.mark.gpu

SIDE, N, NP, M = 6, 21, 6, 2
VECTORS = ("primal", "dual_cone", "dual_eq", "dual_in", "slack_eq", "slack_in")
TRACE_ELAPSED = 12
CAP = 32


def _problem():
    pr = P.maxcut(SIDE, seed=0, avg_degree=3.0)
    (ptr, cols, vals), h = R.triangle_rows(SIDE, [(0, 1, 2)])
    G = sp.csr_matrix((vals[:3 * M], cols[:3 * M], ptr[:M + 1]), shape=(M, pr.n))
    pr = R.with_rows(pr, sp.csc_matrix(G), h[:M])
    assert (pr.n, pr.A.shape[0], pr.G.shape[0]) == (N, NP, M)
    return pr


def _solve(mdl):
    return mdl.solve(factors=True, trace_capacity=CAP)


@pytest.fixture(scope="module")
def kept():
    o = B.default_options()
    B.set_option(o, "max_iter", 30)
    with B.Model(_problem(), o) as mdl:
        r0 = _solve(mdl)
        yield mdl, r0


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda:0")


def _inputs(r0):
    """per method: (call(mdl, a, b), a, b, (the entries a and b must have)) with a, b as NumPy arrays; b None: one input"""
    rng = np.random.default_rng(7)
    x = rng.uniform(-1.0, 1.0, N)                       # (any vector: the separations ask for no PSD matrix)
    vals, V = r0.psd_factors[0][:2]
    assert len(vals) >= 1 and V.shape == (SIDE, len(vals))
    (ptr, cols, addv), addh = R.triangle_rows(SIDE, [(1, 3, 5)])
    ptr, cols, addv, addh = ptr[:2], cols[:3], addv[:3], addh[:1]
    bases = (np.array([[0, 1, 2], [1, 3, 4]]), np.array([[1, 1, -1], [1, -1, 1]]))
    return {
        "update": (lambda m, a, b: m.update(c=a, b=b), rng.standard_normal(N), np.ones(NP), (N, NP)),
        "change_rows": (lambda m, a, b: m.change_rows(add=((ptr, cols, a), b)), addv, addh, (3, 1)),
        "separate_triangles": (lambda m, a, b: m.separate_triangles(a, count=20, min_violation=0.0), x, None, (N,)),
        "separate_cliques": (lambda m, a, b: m.separate_cliques(a, bases, min_violation=0.0), x, None, (N,)),
        "inactive_rows": (lambda m, a, b: m.inactive_rows((a, b)), np.zeros(M), -np.ones(M), (M, M)),
        "round": (lambda m, a, b: m.round((a, b), trials=64), np.asarray(vals), np.asarray(V), None),
        "bound": (lambda m, a, b: m.bound((a, b)), np.zeros(NP), np.zeros(M), (NP, M)),
    }


METHODS = ("update", "change_rows", "separate_triangles", "separate_cliques", "inactive_rows", "round", "bound")
TWO_INPUTS = tuple(k for k in METHODS if k not in ("separate_triangles", "separate_cliques"))


def _counters(mdl):
    i = mdl.info()
    return i["updates"], i["solves"], i["m"]


def _short(a):
    """one entry short (of a matrix: one row short), contiguous"""
    return a[:-1].copy() if isinstance(a, np.ndarray) else a[:-1].contiguous()


@pytest.mark.parametrize("method", TWO_INPUTS)
def test_a_mixture_of_host_arrays_and_cuda_tensors_is_refused_by_name(kept, method):
    mdl, r0 = kept
    call, a, b, _ = _inputs(r0)[method]
    before = _counters(mdl)
    for aa, bb in ((a, _dev(b)), (_dev(a), b)):
        with pytest.raises(ValueError, match=f"Model.{method}: .*cannot be mixed"):
            call(mdl, aa, bb)
    assert _counters(mdl) == before


@pytest.mark.parametrize("method", METHODS)
def test_an_input_one_entry_short_is_refused_on_both_routes(kept, method):
    mdl, r0 = kept
    call, a, b, want = _inputs(r0)[method]
    before = _counters(mdl)
    if method == "round":                               # (the factors are a matrix: a row short, refused by its shape)
        for to in (lambda v: v, _dev):
            with pytest.raises(ValueError, match=f"Model.round: .*{SIDE} x {len(a)}"):
                call(mdl, to(a), _short(to(b)))
        assert _counters(mdl) == before
        return
    pairs = [(_short(a), b, want[0])] + ([(a, _short(b), want[1])] if b is not None else [])
    for aa, bb, count in pairs:
        with pytest.raises(ValueError, match=f"Model.{method}: .*{count}") as e:
            call(mdl, aa, bb)
        assert "entries" in str(e.value)
        with pytest.raises(ValueError, match=f"{count}"):
            call(mdl, _dev(aa), None if bb is None else _dev(bb))
    assert _counters(mdl) == before


def test_the_separations_return_the_same_rows_on_both_routes(kept):
    mdl, r0 = kept
    inp = _inputs(r0)
    before = _counters(mdl)
    call, x, _, _ = inp["separate_triangles"]
    th, td = call(mdl, x, None), call(mdl, _dev(x), None)
    assert len(th) > 0 and th.violated == td.violated and th.scanned == td.scanned
    for k in ("triples", "patterns", "violations"):
        assert np.array_equal(getattr(th, k), getattr(td, k)), k
    for k in th.raw:
        assert np.array_equal(th.raw[k], td.raw[k]), k
    call, x, _, _ = inp["separate_cliques"]
    ch, cd = call(mdl, x, None), call(mdl, _dev(x), None)
    assert len(ch) > 0 and ch.violated_bases == cd.violated_bases and ch.scanned == cd.scanned
    for k in ("nodes", "signs", "violations", "from_base"):
        assert np.array_equal(getattr(ch, k), getattr(cd, k)), k
    for k in ch.raw:
        assert np.array_equal(ch.raw[k], cd.raw[k]), k
    assert _counters(mdl) == before


def test_the_next_solve_returns_the_bits_of_the_solve_before(kept):
    mdl, r0 = kept
    inp = _inputs(r0)
    for method in TWO_INPUTS:                           # (again here, so that this test stands alone)
        call, a, b, _ = inp[method]
        with pytest.raises(ValueError):
            call(mdl, a, _dev(b))
        with pytest.raises(ValueError):
            call(mdl, _short(a), b)
    solves = mdl.info()["solves"]
    r1 = _solve(mdl)
    assert mdl.info()["solves"] == solves + 1
    assert (r1.status, r1.iter, r1.objval, r1.dual_objval) == (r0.status, r0.iter, r0.objval, r0.dual_objval)
    for k in VECTORS:
        assert np.array_equal(np.asarray(getattr(r1, k)), np.asarray(getattr(r0, k))), k
    keep = [c for c in range(B.TRACE_COLS) if c != TRACE_ELAPSED]
    assert r1.trace.shape == r0.trace.shape and np.array_equal(r1.trace[:, keep], r0.trace[:, keep])
    for (v1, V1, i1), (v0, V0, i0) in zip(r1.psd_factors, r0.psd_factors):
        assert np.array_equal(v1, v0) and np.array_equal(V1, V0) and i1 == i0
