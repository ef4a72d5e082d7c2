"""CPU-only tests of the pentagonal / heptagonal separation (proxsdp_hip_model_cliques, proxsdp_host_clique_cuts;
csrc/clique_cuts_host.hpp): the entries are declared and exported and the ABI version stays, the struct has the layout of its
field list, the host restatement equals the NumPy restatement of clique_cases.py exactly -- rows, order, bits, the first
maximum among equal values, the merge of bases that grow into one row, the untouched tail of the output arrays --, and every
refusal that is decided on the host comes back as PROXSDP_E_INVALID before a device is touched."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import clique_cases as K
import triangle_cases as T

E_INVALID = -1
ENTRIES = ("proxsdp_hip_model_cliques", "proxsdp_host_clique_cuts")
SENTINEL = -77
PENTAGON = (1, 4, 5, 8, 11)


def _err():
    return B.lib().proxsdp_hip_last_error().decode(errors="replace")


def test_entries_are_declared_and_exported_and_the_abi_version_stays():
    L = B.lib()
    assert set(ENTRIES) <= set(B.header_symbols())
    for nme in ENTRIES:
        assert hasattr(L, nme), nme
    assert L.proxsdp_hip_abi_version() == 10
    assert callable(B.host_clique_cuts) and callable(B.Model.separate_cliques)
    from proxsdp_jl_amd.optimizer import Optimizer
    assert callable(Optimizer.separate_cliques)


def test_struct_size_follows_the_field_list():
    # int64, 2 x int32 | 4 x int32, int64, 2 doubles | 3 pointers | 7 pointers | 4 x int64, 2 doubles
    assert C.sizeof(B.CliqueCutsIO) == 8 + 2 * 4 + 4 * 4 + 8 + 2 * 8 + 3 * 8 + 7 * 8 + 4 * 8 + 2 * 8
    # and the binding lists the header's members, in order
    import re
    body = re.search(r"typedef struct proxsdp_clique_cuts \{(.*?)\} proxsdp_clique_cuts;", B.HEADER_PATH.read_text(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"(\w+)$", part.strip())[0] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f for f, _ in B.CliqueCutsIO._fields_]


def _host(X, bases, **kw):
    return B.host_clique_cuts(X, bases, sentinel=SENTINEL, **kw)


def _assert_tail_untouched(cuts, n_base, what):
    n, k = len(cuts), cuts.size
    npair = k * (k - 1) // 2
    for name, per in (("nodes", k), ("signs", k), ("violation", 1), ("from_base", 1), ("add_col", npair), ("add_val", npair),
                      ("add_h", 1)):
        a = cuts.arrays[name]
        assert len(a) == per * n_base and np.all(a[per * n:] == SENTINEL), (what, name)


@functools.lru_cache(maxsize=None)
def _triangle_bases(side):
    """all 4 C(side, 3) signed triangles on the small sides; on side 33 every seventh of them"""
    nodes, signs = K.all_triangles(side)
    step = 7 if side > 12 else 1
    return nodes[::step], signs[::step]


@pytest.mark.parametrize("side,rows", [(5, 1), (7, 33), (12, None), (33, None)])
def test_triangles_grow_into_the_pentagons_of_the_restatement(side, rows):
    X = T.gram(side, 3, 0)
    bases = _triangle_bases(side)
    want = K.restatement(X, bases)
    cuts = _host(X, bases)
    K.assert_cliques_equal(cuts, want, side, raw_base=0)
    assert cuts.size == 5 and cuts.bytes_allocated == 0 and cuts.sweep_seconds == 0.0
    if rows is not None:
        assert len(bases[0]) == 4 * len(list(itertools.combinations(range(side), 3))) and len(cuts) == rows
    assert 0 < len(cuts) < cuts.violated_bases <= len(bases[0])      # some bases grow into the same row
    assert np.all(cuts.signs[:, 0] == 1) and np.all(np.diff(cuts.nodes, axis=1) > 0)
    _assert_tail_untouched(cuts, len(bases[0]), side)
    # every row is the inequality it says it is: its left side at X less rhs is the violation, to rounding
    for r in range(len(cuts)):
        assert abs(K.lhs(K._sym(X), cuts.nodes[r], cuts.signs[r]) - 2.0 - cuts.violations[r]) < 1e-12


@pytest.mark.parametrize("side", [7, 12, 33])
def test_pentagons_grow_into_the_heptagons_of_the_restatement(side):
    X = T.gram(side, 3, 0)
    if side == 7:                                                    # the smallest side: every pentagon, alternating signs
        nodes = np.array(list(itertools.combinations(range(7), 5)), dtype=np.int64)
        signs = np.ones_like(nodes, dtype=np.int8)
        signs[:, 1::2] = -1
        bases = (nodes, signs)
        want = K.restatement(X, bases)
    else:                                                            # a CliqueCuts of size 5 is a set of bases
        bases = _host(X, _triangle_bases(side))
        want = K.restatement(X, (bases.nodes, bases.signs))
    cuts = _host(X, bases)
    K.assert_cliques_equal(cuts, want, side, raw_base=0)
    assert cuts.size == 7 and len(cuts) > 0 and np.all(cuts.raw["add_h"] == 3.0)
    _assert_tail_untouched(cuts, len(want["values"]), side)


@pytest.mark.parametrize("side", [7, 70])
def test_equal_values_are_decided_by_the_order_of_the_pairs(side):
    X = T.ties(side)
    ones = lambda n, q: np.ones((n, q), dtype=np.int8)
    tri = np.array([[0, 1, 2], [3, 4, 5], [0, 2, side - 1]], dtype=np.int64)
    cuts = _host(X, (tri, ones(3, 3)))
    K.assert_cliques_equal(cuts, K.restatement(X, (tri, ones(3, 3))), ("ties", side))
    assert np.all(cuts.violations == 3.0) and cuts.from_base.tolist() == [0, 1, 2]
    assert cuts.nodes.tolist() == [[0, 1, 2, 3, 4], [0, 1, 3, 4, 5], [0, 1, 2, 3, side - 1]]
    assert np.all(cuts.signs == 1)
    pent = np.arange(5, dtype=np.int64)[None, :]
    cuts = _host(X, (pent, ones(1, 5)))
    K.assert_cliques_equal(cuts, K.restatement(X, (pent, ones(1, 5))), ("ties, q = 5", side))
    assert cuts.nodes.tolist() == [[0, 1, 2, 3, 4, 5, 6]] and cuts.violations.tolist() == [7.5]


def test_the_triangles_of_a_planted_pentagon_merge_into_one_row():
    X = K.planted(12, PENTAGON)
    tri = np.array(list(itertools.combinations(PENTAGON, 3)), dtype=np.int64)
    bases = (tri, np.ones_like(tri, dtype=np.int8))
    want = K.restatement(X, bases)
    assert np.all(want["values"] > 0.5 - 1e-12)                      # every one of the ten reaches the PSD maximum
    cuts = _host(X, bases)
    K.assert_cliques_equal(cuts, want, "planted")
    assert len(cuts) == 1 and cuts.violated_bases == 10 and cuts.nodes.tolist() == [list(PENTAGON)]
    assert np.all(cuts.signs == 1)
    first_best = int(np.flatnonzero(want["values"] == want["values"].max())[0])
    assert cuts.from_base.tolist() == [first_best] and cuts.violations[0] == want["values"].max()
    _assert_tail_untouched(cuts, 10, "planted")


def test_a_cut_matrix_yields_no_row():
    X = T.feasible(12)
    bases = K.all_triangles(12)
    want = K.restatement(X, bases, min_violation=0.0)
    assert want["values"].max() == 0.0
    cuts = _host(X, bases, min_violation=0.0)
    assert len(cuts) == 0 and cuts.violated_bases == 0 and cuts.scanned == 880 * 4 * 36
    (ptr, cols, vals), h = cuts.add
    assert ptr.tolist() == [0] and len(cols) == 0 and len(vals) == 0 and len(h) == 0
    _assert_tail_untouched(cuts, 880, "feasible")


def test_rhs_threshold_index_base_and_a_variable_list():
    X = T.gram(12, 3, 0)
    bases = _triangle_bases(12)
    for kw in (dict(rhs=1.9), dict(min_violation=0.3), dict(rhs=2.2, min_violation=0.0), dict(index_base=1)):
        K.assert_cliques_equal(_host(X, bases, **kw), K.restatement(X, bases, **kw), kw)
    assert K.restatement(X, bases, min_violation=0.3)["n_rows"] < K.restatement(X, bases)["n_rows"]
    idx = np.random.default_rng(5).permutation(500)[:78].astype(np.int64) + 1      # a cone scattered over 1-based variables
    cuts = _host(X, bases, cone_idx=idx, index_base=1)
    K.assert_cliques_equal(cuts, K.restatement(X, bases, cone_idx=idx), "cone_idx", raw_base=1)
    # only i < j is read
    Y = X.copy()
    Y[np.tril_indices(12)] = np.nan
    K.assert_cliques_equal(_host(Y, bases), K.restatement(X, bases), "upper triangle only")
    # a TriangleCuts is a set of bases: its patterns become the signs of the table
    tc = B.host_triangle_cuts(X, count=40)
    want = K.restatement(X, K.bases_from_triangles(T.brute_force(X, 40)))
    K.assert_cliques_equal(_host(X, tc), want, "from a TriangleCuts")


def test_host_side_refusals():
    L = B.lib()
    X = np.ascontiguousarray(T.gram(7, 3, 0))
    xp = B._p(X)
    host = lambda s, side=7, base=0, x=xp: L.proxsdp_host_clique_cuts(x, side, None, base, C.byref(s))
    model = lambda s: L.proxsdp_hip_model_cliques(None, C.byref(s))
    assert L.proxsdp_host_clique_cuts(xp, 7, None, 0, None) == E_INVALID and "NULL proxsdp_clique_cuts" in _err()
    assert L.proxsdp_hip_model_cliques(None, None) == E_INVALID
    primal = np.zeros(28)

    def damaged(nodes=((0, 1, 2), (1, 3, 4)), signs=((1, -1, 1), (1, 1, -1)), min_violation=1e-3, rhs=None, knobs=None, **kw):
        s, arr = B._clique_struct(np.array(nodes, dtype=np.int64), np.array(signs, dtype=np.int8), min_violation, rhs, knobs)
        s.primal = B._p(primal)
        for k, v in kw.items():
            setattr(s, k, v)
        return s, arr

    cases = {
        "struct_size": (dict(struct_size=C.sizeof(B.CliqueCutsIO) - 8), "struct_size"),
        "base_size 4": (dict(base_size=4), "base_size"),
        "base_size 7": (dict(base_size=7), "base_size"),
        "n_base 0": (dict(n_base=0), "n_base"),
        "n_base too large": (dict(n_base=65537), "n_base"),
        "negative threshold": (dict(min_violation=-1e-9), "min_violation"),
        "nan threshold": (dict(min_violation=np.nan), "min_violation"),
        "inf threshold": (dict(min_violation=np.inf), "min_violation"),
        "inf rhs": (dict(rhs=np.inf), "rhs"),
        "nan rhs": (dict(rhs=np.nan), "rhs"),
        "negative grid": (dict(knobs=dict(grid=-1)), "grid"),
        "negative batch": (dict(knobs=dict(batch=-1)), "batch"),
        "NULL base_nodes": (dict(base_nodes=None), "base_nodes is NULL"),
        "NULL base_sign": (dict(base_sign=None), "base_sign is NULL"),
        "NULL nodes": (dict(nodes=None), "NULL output"),
        "NULL signs": (dict(signs=None), "NULL output"),
        "NULL violation": (dict(violation=None), "NULL output"),
        "NULL from_base": (dict(from_base=None), "NULL output"),
        "NULL add_col": (dict(add_col=None), "NULL output"),
        "NULL add_val": (dict(add_val=None), "NULL output"),
        "NULL add_h": (dict(add_h=None), "NULL output"),
    }
    for name, (kw, text) in cases.items():
        for call in (host, model):
            # (the struct-level keywords nodes / signs of `damaged` are the bases: the output pointers go through setattr)
            outs = {k: kw[k] for k in ("nodes", "signs") if k in kw}
            s, arr = damaged(**{k: v for k, v in kw.items() if k not in outs})
            for k, v in outs.items():
                setattr(s, k, v)
            rc = call(s)
            assert rc == E_INVALID and text in _err(), (name, rc, _err())
    # the bases, which the host entry checks against its side (the model entry needs a handle's cone for them)
    for name, kw, text in (("node past the side", dict(nodes=((0, 1, 2), (1, 3, 7))), "outside the cone"),
                           ("negative node", dict(nodes=((-1, 1, 2), (1, 3, 4))), "outside the cone"),
                           ("equal nodes", dict(nodes=((0, 1, 1), (1, 3, 4))), "not strictly ascending"),
                           ("descending nodes", dict(nodes=((0, 1, 2), (3, 1, 4))), "not strictly ascending"),
                           ("sign 0", dict(signs=((1, 0, 1), (1, 1, -1))), "not +-1"),
                           ("sign 2", dict(signs=((1, 1, 1), (1, 2, -1))), "not +-1"),
                           ("first sign -1", dict(signs=((1, 1, 1), (-1, 1, -1))), "first sign")):
        s, arr = damaged(**kw)
        assert host(s) == E_INVALID and text in _err(), (name, _err())
    # what only the model entry reads
    s, arr = damaged(on_device=2)
    assert model(s) == E_INVALID and "on_device" in _err()
    s, arr = damaged(primal=None)
    assert model(s) == E_INVALID and "primal is NULL" in _err()
    # a request that passes every one of those meets the NULL handle: no model can exist without a device
    s, arr = damaged()
    assert model(s) == E_INVALID and "NULL handle" in _err()
    # what only the host entry reads
    s, arr = damaged()
    assert L.proxsdp_host_clique_cuts(None, 7, None, 0, C.byref(s)) == E_INVALID and "X is NULL" in _err()
    assert host(s, side=4) == E_INVALID and "side" in _err()
    assert host(s, side=46341) == E_INVALID and "side" in _err()
    assert host(s, base=2) == E_INVALID and "index_base" in _err()
    s5, arr5 = damaged(nodes=((0, 1, 2, 3, 4),), signs=((1, 1, 1, 1, 1),))
    assert host(s5, side=6) == E_INVALID and "side" in _err()
    Xn = X.copy()
    Xn[1, 3] = np.inf
    assert host(s, x=B._p(Xn)) == E_INVALID and "non-finite" in _err()
    assert host(s) == 0 and host(s5) == 0 and s5.n_rows <= 1
    with pytest.raises(ValueError):
        B.host_clique_cuts(X, (np.zeros((2, 3)), np.ones((2, 2))))
    with pytest.raises(ValueError):
        B._clique_struct(np.zeros((1, 3), dtype=np.int64), np.ones((1, 3), dtype=np.int8), 1e-3, None, dict(tile=3))


def test_stand_alone_check_of_the_host_half_builds_and_passes(tmp_path):
    """tests/c_harness/clique_cuts_check.cpp: clique_cuts_host.hpp alone, no HIP, no library -- the serial restatement against
    a second brute force in C++ (all extensions sorted, a map for the merge), the total order, the refusals -- built with the
    address and undefined-behaviour sanitizers and run directly.  The sanitizers' runtimes are linked INTO the program: it then
    needs nothing from the environment it is started in, whatever else that environment loads into a process."""
    import pathlib
    import subprocess
    root = pathlib.Path(__file__).resolve().parent.parent
    exe = tmp_path / "clique_cuts_check"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-ffp-contract=off", "-Wall", "-Werror", f"-I{root / 'proxsdp.jl_amd' / 'csrc'}",
           str(root / "tests" / "c_harness" / "clique_cuts_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count(": ok") == 18 and "FAILED" not in r.stdout, r.stdout
