"""CPU checks of the fixtures and references of the vector-kernel tests (vector_kernel_cases.py): the fixtures contain
the shapes they claim, the vectorised column-dot reference is the plain loop, the SOC cases land in the branch their name
says, the derived tolerances already hold between two CPU evaluation orders, and the binding exposes the entries."""
import math

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import vector_kernel_cases as V


def _long_per_block(lens):
    long_ = lens > V.LONGCOL
    nb = -(-len(lens) // V.TPB)
    return [int(long_[b * V.TPB:(b + 1) * V.TPB].sum()) for b in range(nb)]


def test_column_fixture_has_every_length_class():
    cs = V.column_case()
    lens = np.diff(cs["colptr"])
    assert set(V.COL_LENGTHS) <= set(lens.tolist())
    # the classes those lengths stand for (kernels.hip.hpp: LONGCOL = 192, rounds of LC_GROUP = 256, 16-wide chain)
    assert V.LONGCOL in lens and V.LONGCOL + 1 in lens                     # the threshold: last thread column, first wave column
    long_ = lens[lens > V.LONGCOL]
    assert any(L < V.LC_GROUP for L in long_)                              # one round with a clamped tail
    assert any(L < V.LC_GROUP and L % 16 for L in long_) and any(L % 16 == 0 for L in long_)
    assert any(V.LC_GROUP < L <= 2 * V.LC_GROUP for L in long_)            # two rounds
    assert any(L > 3 * V.LC_GROUP for L in long_)                          # both prefetch stages live
    assert any(L % V.LC_GROUP == 0 for L in long_) and any(0 < L % V.LC_GROUP < 16 for L in long_)
    short = lens[lens <= V.LONGCOL]
    assert {0, 1, 3, 4, 5} <= set(short.tolist())                          # col_dot's unrolled-by-four loop and its remainder
    # rows are in random order inside a column (storage order is not sorted order)
    j = int(np.argmax(lens))
    r = cs["row"][cs["colptr"][j]:cs["colptr"][j + 1]]
    assert len(set(r.tolist())) == len(r) and np.any(np.diff(r) < 0)


def test_long_columns_sit_in_the_intended_workgroup_blocks():
    cs = V.column_case()
    lens = np.diff(cs["colptr"])
    assert _long_per_block(lens) == [12, 1, 4, 5, 80, 0]
    assert np.all(lens[1024 + 90:1024 + 170] > V.LONGCOL) and 80 > V.LC_CAP       # adjacent, more than one workgroup takes
    assert len(lens) % V.TPB != 0
    # support order: the wide problem's support is the embedding itself, so support blocks are the logical blocks
    w = V.embed(cs, V.column_keep(cs["n"]))
    S = V.support_of(w)
    assert np.array_equal(S, V.column_keep(cs["n"])) and len(S) < w["n"]
    assert _long_per_block(np.diff(w["colptr"])[S]) == [12, 1, 4, 5, 80, 0]
    assert _long_per_block(np.diff(w["colptr"])) != [12, 1, 4, 5, 80, 0]         # (column order differs from support order)


def test_capped_fixture_is_past_the_grid_cap_with_late_long_columns():
    cs = V.capped_case()
    assert cs["n"] == cs["Q"] == V.GRID_CAP_LEN + 257 > V.PSTRIDE * V.TPB
    lens = np.diff(cs["colptr"])
    longc = np.nonzero(lens > V.LONGCOL)[0]
    assert len(longc) == 4 and longc.min() >= V.GRID_CAP_LEN                      # found in the second pass only
    assert lens.sum() < 20000 and np.count_nonzero(lens) < 4000                   # mostly empty
    w = V.embed(cs, V.capped_keep(cs["n"]))
    S = V.support_of(w)
    assert len(S) == cs["n"] and len(S) < w["n"]
    assert np.searchsorted(S, np.nonzero(np.diff(w["colptr"]) > V.LONGCOL)[0]).min() >= V.GRID_CAP_LEN


def test_special_fixtures_hold_what_their_names_say():
    cs = V.special_case("slack")
    assert np.all(cs["Mx"][cs["p"]:] - cs["bh"][cs["p"]:] < 0)
    assert all(m[8] == 0.0 for m in V.reference(cs)["maxs"])
    cs = V.special_case("ties")
    for i in cs["tie_rows"]:
        bt, th = V.CAND["bt"][i % 3], V.CAND["theta"][i % 3]
        assert (cs["y"][i] + bt * ((1.0 + th) * cs["Mx"][i] - th * cs["Mx_old"][i])) / bt == cs["bh"][i]
    cs = V.special_case("inf")
    assert np.isinf(cs["bh"]).sum() == 5 and np.all(cs["inf_rows"] >= cs["p"])
    assert np.all(np.isfinite(V.reference(cs)["y"]))
    cs = V.special_case("roww")
    assert 0 < np.count_nonzero(cs["roww"] == 0.0) < cs["Q"]
    assert V.special_case("xold0")["xold_coef"] == 0.0
    for k in ("tau", "theta", "bt", "sigma"):                                     # pairwise distinct, no 0.75^k ladder
        v = V.CAND[k]
        assert len(set(v)) == 3 and not math.isclose(v[1] / v[0], 0.75) and not math.isclose(v[2] / v[1], v[1] / v[0])


def test_identity_support_fixtures_have_every_column_in_the_support():
    cases = V.identity_support_cases()
    assert [(cs["Q"], cs["n"]) for cs in cases] == [(1, 1), (64, 64), (65, 65), (257, 257), (300, 130)]
    for cs in cases:
        assert np.all(cs["c"] != 0.0) and cs["roww"] is None                      # (else the GPU test could pass vacuously)
        assert np.array_equal(V.support_of(cs), np.arange(cs["n"]))
    lens = np.diff(cases[-1]["colptr"])
    assert sorted(lens[lens > V.LONGCOL].tolist()) == [V.LONGCOL + 1, 300] and 300 > V.LC_GROUP
    assert all(np.diff(cs["colptr"]).max() <= 5 for cs in cases[:-1])


def test_vectorised_column_dots_are_the_plain_loop():
    cs = V.column_case()
    y = np.random.default_rng(0).standard_normal(cs["Q"])
    fast = V.col_dots(cs["colptr"], cs["row"], cs["val"], y)[0]
    slow = V.col_dots_loop(cs["colptr"], cs["row"], cs["val"], y)
    assert all(fast[j] == v for j, v in slow.items())
    # and a sorted-row or pairwise evaluation is NOT the same bits on the long columns: the order is part of the specification
    j = int(np.argmax(np.diff(cs["colptr"])))
    k = slice(cs["colptr"][j], cs["colptr"][j + 1])
    assert float(np.sum(cs["val"][k] * y[cs["row"][k]])) != fast[j]


@pytest.mark.parametrize("name", ["columns", "capped", "special_roww"])
def test_sum_bound_holds_between_two_cpu_summation_orders(name):
    cs = {"columns": V.column_case, "capped": V.capped_case, "special_roww": lambda: V.special_case("roww")}[name]()
    ref = V.reference(cs, support=(name == "special_roww"))
    worst = 0.0
    for sums in ref["sums"]:
        for q in V.SUM_SLOTS:
            t = sums[q]
            exact, bound = math.fsum(t), V.sum_bound(t)
            pairwise = float(np.sum(t))
            sequential = float(np.cumsum(t)[-1]) if len(t) else 0.0
            assert abs(pairwise - exact) <= bound and abs(sequential - exact) <= bound, (q, pairwise, sequential, exact, bound)
            if bound > 0:
                worst = max(worst, abs(sequential - exact) / bound)
    print(f"{name}: largest |sequential - fsum| / bound = {worst:.3e}")
    assert worst < 1.0


def test_soc_cases_land_in_the_branch_their_name_says():
    x, off, ln, one_off, cases = V.soc_layout()
    assert set(V.SOC_LENGTHS) <= set(ln.tolist())
    assert {b for _, b, _ in cases} == {"polar", "inside", "outside"}
    assert np.any(np.diff(off) < 0)                                               # memory order is not cone order
    ends = off + ln
    order = np.argsort(off)
    assert np.all(off[order][1:] > ends[order][:-1])                              # non-contiguous: a gap before every cone
    for (name, branch, v), o, L in zip(cases, off, ln):
        assert np.array_equal(x[o:o + L].view(np.uint64), v.view(np.uint64))
        got, out, nv, gap = V.soc_reference(v)
        assert got == branch, name
        if not name.startswith(("tie", "len1")):
            assert abs(abs(float(nv)) - abs(float(v[0]))) >= 1e-6 * float(nv), name   # clearly separated
        # float64 NumPy against longdouble stays inside the derived per-entry bound
        err = np.max(np.abs(V.soc_numpy(v).astype(np.longdouble) - out))
        assert float(err) <= V.soc_bound(L, v[0], nv), (name, float(err))
    # the 1x1 blocks sit in the gaps and carry negative, zero, -0.0 and positive values
    inside = np.zeros(len(x), dtype=bool)
    for o, L in zip(off, ln):
        inside[o:o + L] = True
    assert not inside[one_off].any() and len(set(one_off.tolist())) == len(one_off)
    v1 = x[one_off]
    assert (v1 < 0).any() and (v1 > 0).any() and ((v1 == 0) & np.signbit(v1)).any() and ((v1 == 0) & ~np.signbit(v1)).any()


def test_binding_exposes_the_entries():
    assert B.lib().proxsdp_hip_abi_version() == 10
    assert {"proxsdp_hip_trial_batch", "proxsdp_hip_cone_tail"} <= set(B.header_symbols())
    assert hasattr(B.lib(), "proxsdp_hip_trial_batch") and hasattr(B.lib(), "proxsdp_hip_cone_tail")
    assert callable(B.trial_batch) and callable(B.cone_tail)
    assert (B.NCAND, B.NSCAL) == (3, V.NSCAL)
    # the struct mirrors the header: 8 + 8 bytes, 8 pointers, 2 doubles, 4 ints, 14 doubles, 8 pointers, 8 + 4 + 4 bytes
    import ctypes
    assert ctypes.sizeof(B.TrialBatchIO) == 16 + 64 + 16 + 16 + 112 + 64 + 16
