"""The host half of the rounding (proxsdp_host_round, proxsdp_host_round_directions; csrc/rounding_host.hpp;
binding.host_round / host_round_directions): no device.  Every comparison with the NumPy restatement of rounding_cases.py is
an equality -- the contract fixes every fp64 expression -- and the inequalities of the side-16 case stand between exact
numbers (dyadic weights), so no test carries a tolerance."""
import ctypes as C
import pathlib

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import rounding_cases as R

E_INVALID = -1
SIDES = (2, 3, 4, 16, 63, 64, 65, 130)
TRIALS = (64, 128, 192)
SWEEPS = (0, 1, 50)


def _ranks(side):
    """r in {1, 2, 9, 17, s}, the last at side 4"""
    return [r for r in (1, 2, 9, 17) if r <= side] + ([4] if side == 4 else [])


def test_entries_are_declared_and_exported_and_the_abi_version_stays():
    L = B.lib()
    names = set(B.header_symbols())
    for sym in ("proxsdp_hip_model_round", "proxsdp_host_round", "proxsdp_host_round_directions"):
        assert sym in names and hasattr(L, sym), sym
    assert L.proxsdp_hip_abi_version() == 10


def test_struct_size_follows_the_field_list():
    # int64, 4 x int32, int64, 6 x int32 | 9 pointers | 3 x int64, 2 doubles, int64, 2 x int32, int64, 2 doubles
    assert C.sizeof(B.RoundingIO) == 8 + 4 * 4 + 8 + 6 * 4 + 9 * 8 + 3 * 8 + 2 * 8 + 8 + 2 * 4 + 8 + 2 * 8


@pytest.mark.parametrize("r", [1, 2, 17])
@pytest.mark.parametrize("trials", [64, 192])
def test_directions_equal_the_numpy_generator(r, trials):
    for seed in (0, 1234, 2**63 - 1):
        got = B.host_round_directions(seed, r, trials)
        assert got.shape == (r, trials) and np.array_equal(got, R.directions(seed, r, trials)), (seed, r, trials)
    # Irwin-Hall(12) - 6: inside (-6, 6), and not all of one sign
    assert np.all(np.abs(got) < 6.0) and (trials * r < 100 or (got < 0).any() and (got > 0).any())


@pytest.mark.parametrize("side", SIDES)
def test_host_round_equals_the_restatement(side):
    """every r of the side with every sweep limit; the weight type and the number of trials rotate so that each side meets
    both types and all three counts"""
    seen = set()
    for a, r in enumerate(_ranks(side)):
        vals, V = R.factors(side, r, seed=side + r)
        for b, ms in enumerate(SWEEPS):
            kind = ("dyadic", "real")[(a + b) % 2]
            trials = TRIALS[(a + b + side) % 3]
            seen.add((kind, trials))
            cc = R.graph(side, seed=side, kind=kind)
            adj = R.adjacency(cc, side)
            got = B.host_round(vals, V, adj, trials=trials, seed=7 + side, max_sweeps=ms)
            R.assert_rounding_equal(got, R.restate(vals, V, adj, trials, 7 + side, ms), (side, r, ms, kind, trials))
            assert got.bytes_allocated == 0 and got.search_seconds == 0.0 and got.adjacency is None
    assert {k for k, _ in seen} == {"dyadic", "real"} and {t for _, t in seen} == set(TRIALS)


def test_side_16_against_the_brute_force_and_the_tie_rule_on_real_data():
    cc = R.graph(16, seed=16, kind="dyadic")
    adj = R.adjacency(cc, 16)
    vals, V = R.factors(16, 9, seed=25)
    optimum = R.brute_force_minimum(cc, 16)
    for ms in SWEEPS:
        got = B.host_round(vals, V, adj, trials=192, seed=3, max_sweeps=ms)
        assert optimum <= got.value <= got.value_rounded
        assert np.all(got.values_final <= got.values_rounded)
        assert got.value == got.values_final.min() == R.cone_value(cc, got.signs)
        assert got.value_rounded == got.values_rounded.min()
        if ms == 0:
            assert np.array_equal(got.values_final, got.values_rounded) and got.flips == 0 and got.sweeps == 0
    # after the search several trials sit at the same smallest value: the answer is the first of them
    ties = np.nonzero(got.values_final == got.value)[0]
    assert len(ties) > 1 and got.best_trial == ties[0]
    assert got.value == R.cone_value(cc, R.restate(vals, V, adj, 192, 3, 50)["signs"])


def test_an_all_zero_objective_ties_every_trial():
    vals, V = R.factors(16, 2, seed=1)
    got = B.host_round(vals, V, R.adjacency(R.zero_c(16), 16), trials=128, seed=5, max_sweeps=50)
    assert got.best_trial == 0 and got.value == 0.0 and got.flips == 0 and got.sweeps == 1
    assert np.all(got.values_final == 0.0) and np.all(got.values_rounded == 0.0)
    want = R.restate(vals, V, R.adjacency(R.zero_c(16), 16), 128, 5, 50)
    R.assert_rounding_equal(got, want, "zero c")


def test_an_isolated_node_never_flips_and_a_zero_row_rounds_to_plus_one():
    side, iso, zero = 16, (3, 11), 6
    cc = R.graph(side, seed=2, kind="real", isolated=iso)
    adj = R.adjacency(cc, side)
    assert all(adj[0][i + 1] == adj[0][i] for i in iso) and not set(iso) & set(adj[1].tolist())
    vals, V = R.factors(side, 3, seed=4)
    V[zero, :] = 0.0
    before = B.host_round(vals, V, adj, trials=64, seed=9, max_sweeps=0)
    after = B.host_round(vals, V, adj, trials=64, seed=9, max_sweeps=50)
    R.assert_rounding_equal(after, R.restate(vals, V, adj, 64, 9, 50), "isolated")
    assert after.flips > 0
    # the embedding of every trial, restated: an isolated node keeps the sign it was rounded to in the trial that won
    g = R.directions(9, 3, 64)
    y = np.zeros((side, 64))
    for k in range(3):
        y = y + (V[:, k] * np.sqrt(vals)[k])[:, None] * g[k][None, :]
    for i in iso:
        assert (y[i] < 0).any() and (y[i] > 0).any()               # (the node does not round to one sign in every trial)
        assert after.signs[i] == (-1 if y[i, after.best_trial] < 0 else 1)
    # y = 0 in every trial: +1 whichever trial wins, as long as no search moves it
    assert np.all(y[zero] == 0.0) and before.signs[zero] == 1


# ----------------------------------------------------------------- refusals that need no device
def _valid(side=4, r=2, trials=64):
    """a proxsdp_rounding that proxsdp_host_round accepts, its arrays (outputs prefilled with 7), and the adjacency"""
    vals, V = R.factors(side, r, seed=0)
    Q, arr = B._rounding_struct(side, r, trials, 0, 10, sentinel=7)
    arr["V"], arr["vals"] = np.ascontiguousarray(V.T).ravel(), vals
    Q.V, Q.values = B._p(arr["V"]), B._p(arr["vals"])
    ptr, cols, av, diag = R.adjacency(R.graph(side, seed=1), side)
    arr["adj"] = (ptr, cols, av, diag)
    return Q, arr


def _call_host(Q, arr, side=4, adj=None):
    ptr, cols, av, diag = adj if adj is not None else arr["adj"]
    return B.lib().proxsdp_host_round(side, B._p(ptr, B.pi64), B._p(cols, B.pi64), B._p(av), B._p(diag), C.byref(Q))


def _untouched(arr):
    return all(np.all(arr[k] == 7) for k in ("signs", "values_rounded", "values_final"))


def test_host_side_refusals():
    L = B.lib()
    Q, arr = _valid()
    assert _call_host(Q, arr) == 0 and not _untouched(arr)
    ptr, cols, av, diag = arr["adj"]
    assert L.proxsdp_host_round(4, B._p(ptr, B.pi64), B._p(cols, B.pi64), B._p(av), B._p(diag), None) == E_INVALID
    assert L.proxsdp_hip_model_round(None, None) == E_INVALID

    def refused(change, side=4, model=False, adj=None):
        Q, arr = _valid()
        change(Q, arr)
        rc = L.proxsdp_hip_model_round(None, C.byref(Q)) if model else _call_host(Q, arr, side, adj)
        assert rc == E_INVALID and _untouched(arr)
        return L.proxsdp_hip_last_error().decode()

    assert "handle" in refused(lambda Q, a: None, model=True)                      # a NULL handle, everything else valid
    assert "struct_size" in refused(lambda Q, a: setattr(Q, "struct_size", Q.struct_size - 8))
    for f in ("V", "values", "signs"):
        assert "NULL" in refused(lambda Q, a, f=f: setattr(Q, f, None))
    for v in (2, -1):
        assert "on_device" in refused(lambda Q, a, v=v: setattr(Q, "on_device", v), model=True)
    assert "side" in refused(lambda Q, a: setattr(Q, "r", 1), side=1)
    assert "side" in refused(lambda Q, a: None, side=46341)
    for r in (0, -1, 5):
        assert ".r" in refused(lambda Q, a, r=r: setattr(Q, "r", r))
    for t in (0, -64, 63, 100, 65536 + 64):
        assert "trials" in refused(lambda Q, a, t=t: setattr(Q, "trials", t))
    for ms in (-1, 1001):
        assert "max_sweeps" in refused(lambda Q, a, ms=ms: setattr(Q, "max_sweeps", ms))
    assert "knob" in refused(lambda Q, a: setattr(Q, "grid_signs", -1))
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert "values" in refused(lambda Q, a, bad=bad: a["vals"].__setitem__(1, bad))
    for bad in (np.nan, -np.inf):
        assert "V" in refused(lambda Q, a, bad=bad: a["V"].__setitem__(5, bad))
    # the adjacency asked for without its arrays (the model entry decides this before it looks at the handle)
    keep = np.zeros(5, dtype=np.int64)
    assert "adjacency" in refused(lambda Q, a: setattr(Q, "adj_ptr", B._p(keep, B.pi64)), model=True)
    # a malformed adjacency
    two = (np.array([0, 1, 2, 2, 2], dtype=np.int64), np.array([1, 0], dtype=np.int64), np.array([0.5, 0.5]), np.zeros(4))
    assert _call_host(*_valid(), adj=two) == 0
    for k, repl in ((0, [1, 1, 2, 2, 2]), (0, [0, 2, 1, 2, 2]), (1, [0, 0]), (1, [4, 0]), (2, [0.5, np.nan]), (3, [0, np.inf, 0, 0])):
        bad = list(two)
        bad[k] = np.array(repl, dtype=two[k].dtype)
        refused(lambda Q, a: None, adj=tuple(bad))
    descending = (np.array([0, 2, 2, 2, 2], dtype=np.int64), np.array([2, 1], dtype=np.int64), np.array([0.5, 0.5]), np.zeros(4))
    assert "ascend" in refused(lambda Q, a: None, adj=descending)
    # directions
    g = np.full(64, 7.0)
    for seed, r, t, p in ((0, 1, 64, None), (0, 0, 64, g), (0, 46341, 64, g), (0, 1, 32, g), (0, 1, 65600, g)):
        assert L.proxsdp_host_round_directions(seed, r, t, None if p is None else B._p(p)) == E_INVALID
        assert np.all(g == 7.0)
    # the binding's own refusals
    vals, V = R.factors(4, 2, seed=0)
    with pytest.raises(ValueError):
        B.host_round(vals, V[:, :1], arr["adj"])
    with pytest.raises(ValueError):
        B.host_round(vals, V, (ptr[:-1], cols, av, diag))


def test_stand_alone_check_of_the_host_half_builds_and_passes(tmp_path):
    """tests/c_harness/rounding_check.cpp: rounding_host.hpp alone, no HIP, no library -- the serial restatement against a
    second, independent restatement in C++, the adjacency, the tie rule, the refusals.  (The same program is what the address
    and undefined-behaviour sanitizers are pointed at; here it is built plain.)"""
    import subprocess
    root = pathlib.Path(__file__).resolve().parent.parent
    exe = tmp_path / "rounding_check"
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", f"-I{root / 'proxsdp.jl_amd' / 'csrc'}",
           str(root / "tests" / "c_harness" / "rounding_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count(": ok") == 12 and "FAILED" not in r.stdout, r.stdout
