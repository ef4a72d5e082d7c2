"""CPU-only tests of the row change of a model handle (proxsdp_hip_model_rows, proxsdp_host_model_rows_plan;
csrc/model_rows.hip.hpp): the entries are declared and exported, the ABI version stays, the struct has the layout of its
field list, every refusal decided on the host comes back with its code before a device is touched, and the planner's
source and position maps, applied in NumPy to the old model's arrays and the new values, reproduce prepare() of the changed
problem built by hand -- duplicates, empty rows, m = 0 before and after, and a second change on top of the first included."""
import ctypes as C

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P

import kat_problems as K
import model_rows_cases as R

E_INVALID, E_HIP, E_UNSUPP = -1, -2, -4
ENTRIES = ("proxsdp_hip_model_rows", "proxsdp_host_model_rows_plan")


def _err():
    return B.lib().proxsdp_hip_last_error().decode(errors="replace")


def test_entries_are_declared_and_exported_and_the_abi_version_stays():
    L = B.lib()
    names = set(B.header_symbols())
    assert set(ENTRIES) <= names
    for nme in ENTRIES:
        assert hasattr(L, nme), nme
    assert L.proxsdp_hip_abi_version() == 10


def test_struct_size_follows_the_field_list_and_a_wrong_one_is_refused_by_name():
    # int64, 2 x int32 | int64, pointer | int64, 4 pointers | 2 x int64, pointer, 2 x int32, int64, double
    assert C.sizeof(B.ModelRows) == 8 + 2 * 4 + 2 * 8 + 5 * 8 + 2 * 8 + 8 + 2 * 4 + 8 + 8
    L = B.lib()
    s = B.ModelRows()
    s.struct_size = C.sizeof(B.ModelRows) + 8
    assert L.proxsdp_hip_model_rows(None, C.byref(s)) == E_INVALID and "struct_size" in _err()
    s.struct_size = C.sizeof(B.ModelRows)
    assert L.proxsdp_hip_model_rows(None, C.byref(s)) == E_INVALID and "struct_size" not in _err(), _err()


def _rows(drop=None, ptr=None, cols=None, vals=None, h=None, on_device=0):
    """a proxsdp_model_rows over the given arrays (None: NULL), and what keeps them alive"""
    s = B.ModelRows()
    s.struct_size = C.sizeof(B.ModelRows)
    s.on_device = on_device
    keep = []
    if drop is not None:
        keep.append(np.asarray(drop, dtype=np.int64)); s.n_drop, s.drop = len(drop), B._p(keep[-1], B.pi64)
    if ptr is not None:
        keep.append(np.asarray(ptr, dtype=np.int64)); s.n_add, s.add_ptr = len(ptr) - 1, B._p(keep[-1], B.pi64)
    if cols is not None:
        keep.append(np.asarray(cols, dtype=np.int64)); s.add_col = B._p(keep[-1], B.pi64)
    if vals is not None:
        keep.append(np.asarray(vals, dtype=np.float64)); s.add_val = B._p(keep[-1])
    if h is not None:
        keep.append(np.asarray(h, dtype=np.float64)); s.add_h = B._p(keep[-1])
    return s, keep


def test_refusals_that_need_no_model_are_decided_before_the_handle():
    L = B.lib()
    call = lambda s: L.proxsdp_hip_model_rows(None, C.byref(s))
    assert L.proxsdp_hip_model_rows(None, None) == E_INVALID
    good = dict(ptr=[0, 2], cols=[0, 1], vals=[1.0, 2.0], h=[1.0])
    cases = {
        "both 0": (dict(), "both 0"),
        "on_device": (dict(good, on_device=2), "on_device"),
        "drop is NULL": (dict(), "drop is NULL"),
        "add_h is NULL": (dict(good, h=None), "add_h"),
        "add_col is NULL": (dict(good, cols=None), "add_col"),
        "add_val is NULL": (dict(good, vals=None), "add_col / add_val"),
        "add_ptr[0]": (dict(good, ptr=[1, 2]), "add_ptr[0]"),
        "monotone": (dict(good, ptr=[0, 2, 1], h=[1.0, 1.0]), "monotone"),
        "nan value": (dict(good, vals=[1.0, np.nan]), "non-finite entry in add_val"),
        "inf h": (dict(good, h=[np.inf]), "non-finite entry in add_h"),
    }
    for name, (kw, text) in cases.items():
        s, keep = _rows(**kw)
        if name == "drop is NULL":
            s.n_drop = 2
        rc = call(s)
        assert rc == E_INVALID and rc != E_HIP and text in _err(), (name, rc, _err())
    # a change that passes every one of those meets the NULL handle: no model can exist without a device
    s, keep = _rows(**good)
    assert call(s) == E_INVALID and "NULL handle" in _err()
    s, keep = _rows(drop=[0])
    assert call(s) == E_INVALID and "NULL handle" in _err()
    # add_ptr given but n_add = 0 and n_drop = 0
    s, keep = _rows(ptr=[0])
    assert call(s) == E_INVALID and "both 0" in _err()


def test_refusals_that_need_the_model_are_decided_by_the_planner_on_the_host():
    """the planner is the first thing proxsdp_hip_model_rows runs on a handle: its refusals through the host entry"""
    L = B.lib()
    pr = K.mixed_cones()
    M = B._Marshalled(pr)
    D = B.ModelDump()
    D.struct_size = C.sizeof(B.ModelDump)
    plan = lambda s: L.proxsdp_host_model_rows_plan(C.byref(M.P), C.byref(s), C.byref(D), None, None, None, None, None)
    m, n = pr.G.shape
    cases = {
        "drop below": (dict(drop=[-1]), "out of range"),
        "drop above": (dict(drop=[m]), "out of range"),
        "drop repeated": (dict(drop=[3, 5, 3]), "repeated"),
        "column above": (dict(ptr=[0, 1], cols=[n], vals=[1.0], h=[0.0]), "column out of range"),
        "column below": (dict(ptr=[0, 1], cols=[-1], vals=[1.0], h=[0.0]), "column out of range"),
    }
    for name, (kw, text) in cases.items():
        s, keep = _rows(**kw)
        rc = plan(s)
        assert rc == E_INVALID and text in _err(), (name, rc, _err())
    s, keep = _rows(drop=[0], on_device=1)
    assert plan(s) == E_INVALID and "host values" in _err()
    s, keep = _rows(drop=[0])
    D.struct_size += 8
    assert plan(s) == E_INVALID and "proxsdp_model_dump.struct_size" in _err()
    D.struct_size -= 8
    assert plan(s) == 0, _err()
    assert (s.m_new, D.Q) == (m - 1, pr.A.shape[0] + m - 1)
    # with index base 1 the columns follow it, the drop numbers stay 0-based
    M1 = B._Marshalled(pr, None, 1)
    plan1 = lambda s: L.proxsdp_host_model_rows_plan(C.byref(M1.P), C.byref(s), C.byref(D), None, None, None, None, None)
    s, keep = _rows(drop=[0], ptr=[0, 1], cols=[0], vals=[1.0], h=[0.0])
    assert plan1(s) == E_INVALID and "column out of range" in _err()
    s, keep = _rows(drop=[0], ptr=[0, 1], cols=[n], vals=[1.0], h=[0.0])
    assert plan1(s) == 0, _err()


# ----------------------------------------------------------------- the planner
DUMP_VALUES = ("csc_val", "csr_val", "csc_val_orig", "csr_val_orig")


def _apply_maps(old, plan, add, cte_of_t):
    """the new arrays from the old model's arrays and the new values through the planner's source maps, in NumPy"""
    vals = np.zeros(0) if add is None else np.asarray(add[0][2], dtype=np.float64)
    h_new = np.zeros(0) if add is None else np.asarray(add[1], dtype=np.float64)
    scaled = vals * cte_of_t                                     # one product per new entry, as the kernel forms it
    out = {}
    for name, src in (("csc_val", "csc_src"), ("csr_val", "csr_src"), ("csc_val_orig", "csc_src"), ("csr_val_orig", "csr_src")):
        s = plan[src]
        new = scaled if name in ("csc_val", "csr_val") else vals
        a = np.zeros(len(s))
        a[s >= 0] = old[name][s[s >= 0]]
        a[s < 0] = new[-1 - s[s < 0]]
        out[name] = a
    s = plan["bh_src"]
    bh = np.zeros(len(s))
    bh[s >= 0] = old["bh"][s[s >= 0]]
    bh[s < 0] = h_new[-1 - s[s < 0]]
    out["bh"] = bh
    return out


def _offdiag_by_variable(pr):
    od = np.zeros(pr.n, dtype=bool)
    for side, idx in zip(pr.psd_sides(), pr.psd):
        k = 0
        for j in range(side):
            for i in range(j + 1):
                od[idx[k]] = i != j
                k += 1
    return od


def _check_change(pr, add, drop, what):
    """plan the change on `pr`, compare with prepare() of the problem built by hand; returns the changed problem"""
    G2, h2, kept, _ = R.stack_rows(pr.G, pr.h, add, drop)
    pr2 = R.with_rows(pr, G2, h2)
    old, want = B.host_model_prepare(pr), B.host_model_prepare(pr2)
    plan = B.host_model_rows_plan(pr, add=add, drop=drop)
    assert np.array_equal(plan["kept"], kept) and plan["m"] == G2.shape[0], what
    cte = np.sqrt(2.0) / 2.0
    cols = np.zeros(0, dtype=np.int64) if add is None else np.asarray(add[0][1])
    cte_of_t = np.where(_offdiag_by_variable(pr)[cols], cte, 1.0)
    got = _apply_maps(old, plan, add, cte_of_t)
    for k in DUMP_VALUES + ("bh",):
        assert np.array_equal(got[k], want[k]), (what, k, "through the source maps")
    for k, _ in B.MODEL_DUMP_ARRAYS:
        assert np.array_equal(plan[k], want[k]), (what, k, "the planner's dump")
    for k in ("n", "Q", "nnz", "ns"):
        assert plan[k] == want[k], (what, k)
    for k in ("csc_pos", "csr_pos"):
        assert np.array_equal(plan[k], want[k]), (what, k)
    for k in B.MODEL_NORM_NAMES:
        assert plan[k] == want[k], (what, k, plan[k], want[k])
    # every kept position is read once, every new entry once
    for k in ("csc_src", "csr_src"):
        s = plan[k]
        assert len(set(s[s >= 0])) == int((s >= 0).sum()) and sorted(-1 - s[s < 0]) == list(range(len(cols))), (what, k)
    return pr2


@pytest.mark.parametrize("seed", [0, 1])
def test_planner_on_the_models_with_duplicates_and_a_second_change_on_top(seed):
    pr = R.random_with_duplicates(seed)
    add = R.duplicate_rows(pr.n, seed)
    pr2 = _check_change(pr, add, [0, 2], ("duplicates", seed, "first change"))
    assert pr2.G.shape[0] == 4 - 2 + 3
    # the maps compose: a second change on the changed model (drop a kept row and the empty new one, add one row)
    add2 = ((np.array([0, 2]), np.array([1, 1]), np.array([0.5, -2.0])), np.array([0.25]))
    pr3 = _check_change(pr2, add2, [1, 3], ("duplicates", seed, "second change"))
    assert pr3.G.shape[0] == 5 - 2 + 1


def test_planner_dropping_every_row_of_the_mixed_model():
    pr = K.mixed_cones()
    pr2 = _check_change(pr, None, list(range(12))[::-1], "mixed cones, m' = 0")
    assert pr2.G.shape[0] == 0 and pr2.G.nnz == 0


def test_planner_from_no_rows_to_eight_triangle_rows():
    pr = P.maxcut(12, seed=0)
    assert pr.G.shape[0] == 0
    add = R.triangle_rows(12, R.first_triples(12, 2))
    pr2 = _check_change(pr, add, None, "maxcut12, m 0 -> 8")
    assert pr2.G.shape == (8, pr.n) and pr2.G.nnz == 24
    # and a drop with an add on top of it
    add2 = R.triangle_rows(12, [(3, 7, 11)])
    _check_change(pr2, add2, [0, 5, 6], "maxcut12, second change")


def test_python_change_rows_refuses_mixed_host_and_device_values():
    class FakeCuda:                                             # what binding._is_tensor looks for
        is_cuda = True

        def data_ptr(self):
            return 0

    mdl = B.Model.__new__(B.Model)
    mdl.n, mdl.p, mdl.m, mdl._nnz, mdl._h = 3, 1, 0, (1, 0), None
    with pytest.raises(ValueError, match="mixed"):
        mdl.change_rows(add=((np.array([0, 1]), np.array([0]), np.array([1.0])), FakeCuda()))
    with pytest.raises(ValueError, match="mixed"):
        mdl.change_rows(add=((np.array([0, 1]), np.array([0]), FakeCuda()), np.array([1.0])))
