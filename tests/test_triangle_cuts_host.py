"""CPU-only tests of the triangle separation and the slack-row entry (proxsdp_hip_model_triangles,
proxsdp_host_triangle_cuts, proxsdp_hip_model_inactive_rows; csrc/triangle_cuts.hip.hpp): the entries are declared and
exported and the ABI version stays, the structs have the layout of their field lists, the host restatement equals the NumPy
brute force of triangle_cases.py exactly -- rows, order, bits, the cut-off among equal violations, the untouched tail of the
output arrays --, and every refusal that is decided on the host comes back as PROXSDP_E_INVALID before a device is touched."""
import ctypes as C

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import triangle_cases as T

E_INVALID, E_HIP = -1, -2
ENTRIES = ("proxsdp_hip_model_triangles", "proxsdp_host_triangle_cuts", "proxsdp_hip_model_inactive_rows")
SENTINEL = -77
CASES = {3: (2, 0), 4: (2, 0), 12: (3, 0), 65: (3, 1)}              # side: (r, seed) of gram
VIOLATED = {3: 1, 4: 4, 12: 157, 65: 28947}                          # at min_violation = 1e-3, rhs = 1 (NumPy, checked below)


def _err():
    return B.lib().proxsdp_hip_last_error().decode(errors="replace")


def test_entries_are_declared_and_exported_and_the_abi_version_stays():
    L = B.lib()
    names = set(B.header_symbols())
    assert set(ENTRIES) <= names
    for nme in ENTRIES:
        assert hasattr(L, nme), nme
    assert L.proxsdp_hip_abi_version() == 10
    assert callable(B.host_triangle_cuts) and callable(B.Model.separate_triangles) and callable(B.Model.inactive_rows)
    from proxsdp_jl_amd.optimizer import Optimizer
    assert callable(Optimizer.separate_triangles) and callable(Optimizer.inactive_rows)


def test_struct_sizes_follow_the_field_lists():
    # int64, 2 x int32, int64, 2 doubles, int64, pointer | 6 pointers | 3 x int64, 2 x int32, int64, 2 doubles
    assert C.sizeof(B.TriangleCutsIO) == 8 + 2 * 4 + 8 + 2 * 8 + 8 + 8 + 6 * 8 + 3 * 8 + 2 * 4 + 8 + 2 * 8
    # int64, 2 x int32, 2 pointers, 2 doubles, pointer, int64
    assert C.sizeof(B.InactiveRowsIO) == 8 + 2 * 4 + 2 * 8 + 2 * 8 + 8 + 8


def test_the_fixtures_are_what_the_brute_force_says_they_are():
    for side, (r, seed) in CASES.items():
        X = T.gram(side, r, seed)
        _, V = T.all_rows(X)
        v = V[V > 1e-3]
        assert len(v) == VIOLATED[side] and V.size == 4 * side * (side - 1) * (side - 2) // 6, side
        assert len(np.unique(v)) == len(v), side                    # all violated values are pairwise distinct
    Tt, V = T.all_rows(T.ties(12))
    assert np.all(V[:, 0] == 0.5) and np.all(V[:, 1:] <= 0.0)
    _, V = T.all_rows(T.feasible(12))
    assert np.all(V <= 0.0)


def _host(X, count, **kw):
    return B.host_triangle_cuts(X, count=count, sentinel=SENTINEL, **kw)


def _assert_tail_untouched(cuts, count, what):
    k = len(cuts)
    for name, per in (("tri", 3), ("pattern", 1), ("violation", 1), ("add_col", 3), ("add_val", 3), ("add_h", 1)):
        a = cuts.arrays[name]
        assert len(a) == per * count and np.all(a[per * k:] == SENTINEL), (what, name)


@pytest.mark.parametrize("side", sorted(CASES))
def test_host_entry_equals_the_brute_force(side):
    X = T.gram(side, *CASES[side])
    nv = VIOLATED[side]
    for count in sorted({1, 5, nv, nv + 7}):
        cuts = _host(X, count)
        want = T.brute_force(X, count)
        T.assert_cuts_equal(cuts, want, (side, count), raw_base=0)
        assert len(cuts) == min(count, nv) and cuts.passes == 0
        _assert_tail_untouched(cuts, count, (side, count))


def test_equal_violations_are_cut_off_by_the_index_order():
    X = T.ties(12)
    cuts = _host(X, 5)
    T.assert_cuts_equal(cuts, T.brute_force(X, 5), "ties")
    assert cuts.violated == 220 and np.all(cuts.violations == 0.5) and np.all(cuts.patterns == 0)
    assert cuts.triples.tolist() == [[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 5], [0, 1, 6]]
    # more rows than the trimming buffer of the partial sort holds at once
    cuts = _host(T.ties(40), 3)
    assert cuts.violated == 9880 and cuts.triples.tolist() == [[0, 1, 2], [0, 1, 3], [0, 1, 4]]


def test_a_cut_matrix_violates_nothing():
    cuts = _host(T.feasible(12), 10)
    assert len(cuts) == 0 and cuts.violated == 0 and cuts.scanned == 880
    _assert_tail_untouched(cuts, 10, "feasible")


def test_rhs_threshold_index_base_and_a_variable_list():
    X = T.gram(12, 3, 0)
    for kw in (dict(rhs=0.9), dict(min_violation=0.2), dict(rhs=1.1, min_violation=0.0), dict(index_base=1)):
        T.assert_cuts_equal(_host(X, 40, **kw), T.brute_force(X, 40, **kw), kw)
    assert T.brute_force(X, 1000, min_violation=0.2)["violated"] < VIOLATED[12]
    idx = np.random.default_rng(5).permutation(500)[:78].astype(np.int64) + 1      # a cone scattered over 1-based variables
    cuts = _host(X, 40, cone_idx=idx, index_base=1)
    T.assert_cuts_equal(cuts, T.brute_force(X, 40, cone_idx=idx), "cone_idx", raw_base=1)
    # only i < j is read
    Y = X.copy()
    Y[np.tril_indices(12)] = np.nan
    T.assert_cuts_equal(_host(Y, 40), T.brute_force(X, 40), "upper triangle only")


def _struct(count=4, min_violation=1e-3, rhs=1.0, cand_cap=0):
    return B._triangle_struct(count, min_violation, rhs, cand_cap)


def test_host_side_refusals_of_the_separation():
    L = B.lib()
    X = np.ascontiguousarray(T.gram(4, 2, 0))
    xp = B._p(X)
    host = lambda s, side=4, base=0, x=xp: L.proxsdp_host_triangle_cuts(x, side, None, base, C.byref(s))
    model = lambda s: L.proxsdp_hip_model_triangles(None, C.byref(s))
    assert L.proxsdp_host_triangle_cuts(xp, 4, None, 0, None) == E_INVALID
    assert L.proxsdp_hip_model_triangles(None, None) == E_INVALID
    primal = np.zeros(10)

    def damaged(**kw):
        s, arr = _struct(**{k: v for k, v in kw.items() if k in ("count", "min_violation", "rhs", "cand_cap")})
        s.primal = B._p(primal)
        for k, v in kw.items():
            if k not in ("count", "min_violation", "rhs", "cand_cap"):
                setattr(s, k, v)
        return s, arr

    cases = {
        "struct_size": (dict(struct_size=C.sizeof(B.TriangleCutsIO) - 8), "struct_size"),
        "count 0": (dict(count=0), "count"),
        "count too large": (dict(count=(1 << 20) + 1), "count"),
        "negative threshold": (dict(min_violation=-1e-9), "min_violation"),
        "nan threshold": (dict(min_violation=np.nan), "min_violation"),
        "inf threshold": (dict(min_violation=np.inf), "min_violation"),
        "inf rhs": (dict(rhs=np.inf), "rhs"),
        "nan rhs": (dict(rhs=np.nan), "rhs"),
        "negative cand_cap": (dict(cand_cap=-1), "cand_cap"),
        "NULL tri": (dict(tri=None), "NULL output"),
        "NULL pattern": (dict(pattern=None), "NULL output"),
        "NULL violation": (dict(violation=None), "NULL output"),
        "NULL add_col": (dict(add_col=None), "NULL output"),
        "NULL add_val": (dict(add_val=None), "NULL output"),
        "NULL add_h": (dict(add_h=None), "NULL output"),
    }
    for name, (kw, text) in cases.items():
        for call in (host, model):
            s, arr = damaged(**kw)
            rc = call(s)
            assert rc == E_INVALID and text in _err(), (name, rc, _err())
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
    assert L.proxsdp_host_triangle_cuts(None, 4, None, 0, C.byref(s)) == E_INVALID and "X is NULL" in _err()
    assert host(s, side=2) == E_INVALID and "side" in _err()
    assert host(s, base=2) == E_INVALID and "index_base" in _err()
    Xn = X.copy()
    Xn[1, 3] = np.inf
    assert host(s, x=B._p(Xn)) == E_INVALID and "non-finite" in _err()
    assert host(s) == 0 and s.n_rows == 4 and s.violated == 4


def test_stand_alone_check_of_the_host_half_builds_and_passes(tmp_path):
    """tests/c_harness/triangle_cuts_check.cpp: triangle_cuts_host.hpp alone, no HIP, no library -- the serial restatement
    against a second brute force in C++, the gate of a later sweep against the prefix test it replaces, the slack rows of
    host vectors.  (The same program is what the address and undefined-behaviour sanitizers are pointed at; here it is built
    plain.)"""
    import pathlib
    import subprocess
    root = pathlib.Path(__file__).resolve().parent.parent
    exe = tmp_path / "triangle_cuts_check"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", f"-I{root / 'proxsdp.jl_amd' / 'csrc'}",
           str(root / "tests" / "c_harness" / "triangle_cuts_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count(": ok") == 13 and "FAILED" not in r.stdout, r.stdout


def test_host_side_refusals_of_the_slack_rows():
    L = B.lib()
    call = lambda q: L.proxsdp_hip_model_inactive_rows(None, C.byref(q))
    assert L.proxsdp_hip_model_inactive_rows(None, None) == E_INVALID
    d, s, rows = np.zeros(3), np.zeros(3), np.zeros(3, dtype=np.int64)

    def request(**kw):
        q = B.InactiveRowsIO()
        q.struct_size = C.sizeof(B.InactiveRowsIO)
        q.dual_in, q.slack_in, q.rows = B._p(d), B._p(s), B._p(rows, B.pi64)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    for name, kw, text in (("struct_size", dict(struct_size=8), "struct_size"), ("on_device", dict(on_device=3), "on_device"),
                           ("dual", dict(dual_in=None), "NULL array"), ("slack", dict(slack_in=None), "NULL array"),
                           ("rows", dict(rows=None), "NULL array"), ("negative", dict(dual_tol=-1.0), "dual_tol"),
                           ("nan", dict(slack_tol=np.nan), "slack_tol"), ("inf", dict(dual_tol=np.inf), "dual_tol")):
        rc = call(request(**kw))
        assert rc == E_INVALID and text in _err(), (name, rc, _err())
    assert call(request()) == E_INVALID and "NULL handle" in _err()
