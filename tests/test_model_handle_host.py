"""CPU-only tests of the model handle's boundary (proxsdp_hip_model_*, include/proxsdp_hip.h): the entries are declared and
exported, the ABI version stays, the three new structs have the layout of their field lists, every refusal that is decided on
the host comes back with its code before a device is touched (never PROXSDP_E_HIP on a machine without one), and the position
maps prepare() records for a handle reproduce a second prepare() on changed values -- duplicates inside a column included."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from proxsdp_jl_amd import binding as B
from proxsdp_jl_amd import problems as P

import kat_problems as K

E_INVALID, E_HIP, E_UNSUPP = -1, -2, -4
ENTRIES = ("proxsdp_hip_model_create", "proxsdp_hip_model_update", "proxsdp_hip_model_solve", "proxsdp_hip_model_info",
           "proxsdp_hip_model_destroy", "proxsdp_hip_model_dump")


def _err():
    return B.lib().proxsdp_hip_last_error().decode(errors="replace")


def test_entries_are_declared_and_exported_and_the_abi_version_stays():
    L = B.lib()
    names = set(B.header_symbols())
    assert set(ENTRIES) <= names
    for nme in ENTRIES:
        assert hasattr(L, nme), nme
    assert L.proxsdp_hip_abi_version() == 10


def test_struct_sizes_follow_their_field_lists():
    # proxsdp_model_data: int64, 2 x int32, 5 pointers; _info: 6 x int64, 2 x int32, 4 x int64, double;
    # _dump: 5 x int64, 9 pointers, 4 doubles
    assert C.sizeof(B.ModelData) == 8 + 2 * 4 + 5 * 8
    assert C.sizeof(B.ModelInfo) == 6 * 8 + 2 * 4 + 4 * 8 + 8
    assert C.sizeof(B.ModelDump) == 5 * 8 + 9 * 8 + 4 * 8
    L = B.lib()
    # the C side's sizeof is the one its struct_size check accepts: checked before the handle, so NULL serves
    for struct, call in ((B.ModelData, lambda s: L.proxsdp_hip_model_update(None, C.byref(s))),
                         (B.ModelInfo, lambda s: L.proxsdp_hip_model_info(None, C.byref(s))),
                         (B.ModelDump, lambda s: L.proxsdp_hip_model_dump(None, C.byref(s)))):
        s = struct()
        s.struct_size = C.sizeof(struct) + 8
        assert call(s) == E_INVALID and "struct_size" in _err(), struct.__name__
        s.struct_size = C.sizeof(struct)
        assert call(s) == E_INVALID and "struct_size" not in _err(), (struct.__name__, _err())


def test_null_arguments_are_refused_on_the_host():
    L = B.lib()
    M = B._Marshalled(K.sdp_wiki(False))
    o = B.default_options()
    h = C.c_void_p()
    assert L.proxsdp_hip_model_create(None, C.byref(o), C.byref(h)) == E_INVALID
    assert L.proxsdp_hip_model_create(C.byref(M.P), C.byref(o), None) == E_INVALID
    R = B.Result()
    assert L.proxsdp_hip_model_solve(None, None, C.byref(R), None, None, None, None) == E_INVALID
    assert L.proxsdp_hip_model_update(None, None) == E_INVALID
    assert L.proxsdp_hip_model_info(None, None) == E_INVALID
    assert L.proxsdp_hip_model_dump(None, None) == E_INVALID
    assert L.proxsdp_hip_model_destroy(None) == 0


def test_create_refuses_a_wrong_options_size_before_the_device():
    L = B.lib()
    M = B._Marshalled(K.sdp_wiki(False))
    o = B.default_options()
    o.struct_size += 8
    h = C.c_void_p()
    assert L.proxsdp_hip_model_create(C.byref(M.P), C.byref(o), C.byref(h)) == E_INVALID
    assert "struct_size" in _err() and not h.value


def test_create_refuses_a_shard_a_dense_matrix_and_the_warmup_as_unsupported():
    L = B.lib()
    o = B.default_options()
    h = C.c_void_p()
    M = B._Marshalled(K.sdp_wiki(False))
    cb = B.REDUCE_FN(lambda ctx, ps, ns, pm, nm: 0)
    M.P.reduce_fn = C.cast(cb, C.c_void_p)
    assert L.proxsdp_hip_model_create(C.byref(M.P), C.byref(o), C.byref(h)) == E_UNSUPP
    assert "shard" in _err()
    M = B._Marshalled(K.sdp_wiki(False))
    rows = np.zeros(1, dtype=np.int64)
    owned = np.ones(1, dtype=np.int32)
    M.P.n_coupling, M.P.coupling_rows, M.P.coupling_owned = 1, B._p(rows, B.pi64), owned.ctypes.data_as(C.POINTER(B.i32))
    assert L.proxsdp_hip_model_create(C.byref(M.P), C.byref(o), C.byref(h)) == E_UNSUPP
    assert "shard" in _err()
    M = B._Marshalled(P.randsdp(5, 4, seed=2, dense=True))
    assert M.P.M_dense
    assert L.proxsdp_hip_model_create(C.byref(M.P), C.byref(o), C.byref(h)) == E_UNSUPP
    assert "M_dense" in _err()
    M = B._Marshalled(K.sdp_wiki(False))
    B.set_option(o, "rocsolver_warmup", 1)
    assert L.proxsdp_hip_model_create(C.byref(M.P), C.byref(o), C.byref(h)) == E_UNSUPP
    assert "rocsolver_warmup" in _err() and not h.value


def test_create_applies_the_argument_checks_of_solve_on_the_host():
    L = B.lib()
    o = B.default_options()
    h = C.c_void_p()
    M = B._Marshalled(K.sdp_wiki(False))
    M.P.index_base = 2
    assert L.proxsdp_hip_model_create(C.byref(M.P), C.byref(o), C.byref(h)) == E_INVALID
    msg = _err()
    R = B.Result()
    assert L.proxsdp_hip_solve(C.byref(M.P), C.byref(o), C.byref(R)) == E_INVALID and _err() == msg


def test_update_refusals_decided_on_the_host():
    L = B.lib()
    D = B.ModelData()
    D.struct_size = C.sizeof(B.ModelData)
    assert L.proxsdp_hip_model_update(None, C.byref(D)) == E_INVALID and "every pointer is NULL" in _err()
    bad = np.array([1.0, np.nan])
    D.c = B._p(bad)
    rc = L.proxsdp_hip_model_update(None, C.byref(D))          # no handle can exist without a device: refused as such
    assert rc == E_INVALID and rc != E_HIP
    D.on_device = 2
    assert L.proxsdp_hip_model_update(None, C.byref(D)) == E_INVALID and "on_device" in _err()


def test_python_update_refuses_mixed_host_and_device_arguments():
    class FakeCuda:                                             # what binding._is_tensor looks for
        is_cuda = True

        def data_ptr(self):
            return 0

    mdl = B.Model.__new__(B.Model)
    mdl.n, mdl.p, mdl.m, mdl._nnz, mdl._h = 2, 1, 0, (1, 0), None
    with pytest.raises(ValueError, match="mixed"):
        mdl.update(c=np.zeros(2), b=FakeCuda())


def test_no_cpu_fallback_without_a_device():
    if B.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(B.ProxSDPHipError) as e:
        B.Model(K.sdp_wiki(False))
    assert e.value.code == E_HIP


# ----------------------------------------------------------------- the position maps
def _offdiag_in_solver_order(prob):
    """per position of the solver's order: is it an off-diagonal entry of a PSD cone (cones first, in cone order)"""
    od = []
    for side in prob.psd_sides():
        for j in range(side):
            for i in range(j + 1):
                od.append(i != j)
    return np.array(od + [False] * (prob.n - len(od)))


def _solver_order(prob):
    M = B._Marshalled(prob)
    order = np.zeros(max(prob.n, 1), dtype=np.int64)
    B._check(B.lib().proxsdp_host_preprocess(C.byref(M.P), B._p(order, B.pi64), None, None, None))
    return order[:prob.n]


def _random_with_duplicates(seed):
    """a small model with two PSD cones, one SOC and free variables, the variables not in solver order, and columns of A
    and G that store the same row more than once"""
    rng = np.random.default_rng(seed)
    sides = (3, 1, 4)
    lens = [s * (s + 1) // 2 for s in sides]
    n = sum(lens) + 3 + 2
    perm = rng.permutation(n)
    psd, pos = [], 0
    for ln in lens:
        psd.append(perm[pos:pos + ln].astype(np.int64)); pos += ln
    soc = [perm[pos:pos + 3].astype(np.int64)]

    def mat(rows):
        indptr, indices = [0], []
        for j in range(n):
            cnt = int(rng.integers(0, 4))
            r = rng.integers(0, rows, cnt)
            if cnt >= 2 and rng.random() < 0.5:
                r[1] = r[0]                                        # a duplicate inside the column
            indices += sorted(int(v) for v in r)
            indptr.append(len(indices))
        data = rng.standard_normal(len(indices))
        return sp.csc_matrix((data, np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)), shape=(rows, n))

    A, G = mat(5), mat(4)
    assert not A.has_canonical_format or not G.has_canonical_format, "the pattern has no duplicate"
    c = rng.standard_normal(n) * (rng.random(n) < 0.7)
    return P.Problem(n=n, A=A, b=rng.standard_normal(5), G=G, h=rng.standard_normal(4), c=c, psd=psd, soc=soc)


def _stored(M):
    M = sp.csc_matrix(M, dtype=np.float64)
    M.sort_indices()
    return M.data.copy()


@pytest.mark.parametrize("make", [lambda: _random_with_duplicates(0), lambda: _random_with_duplicates(1),
                                  lambda: K.mixed_cones(), lambda: P.maxcut(12, seed=0)],
                         ids=["duplicates0", "duplicates1", "mixed_cones", "maxcut12"])
def test_position_maps_reproduce_a_second_prepare_on_changed_values(make):
    pr = make()
    base = B.host_model_prepare(pr)
    nA = len(_stored(pr.A))
    assert base["nnz_A"] == nA and base["nnz"] == nA + len(_stored(pr.G))
    cp, rp = base["csc_pos"], base["csr_pos"]
    assert sorted(cp) == list(range(base["nnz"])) and sorted(rp) == list(range(base["nnz"]))
    rng = np.random.default_rng(7)
    A2, G2 = sp.csc_matrix(pr.A, dtype=np.float64), sp.csc_matrix(pr.G, dtype=np.float64)
    A2.sort_indices(); G2.sort_indices()
    A2.data = rng.standard_normal(len(A2.data)); G2.data = rng.standard_normal(len(G2.data))
    c2 = rng.standard_normal(pr.n)
    pr2 = P.Problem(n=pr.n, A=A2, b=pr.b + 1.0, G=G2, h=pr.h - 1.0, c=c2, psd=pr.psd, soc=pr.soc)
    want = B.host_model_prepare(pr2)
    assert np.array_equal(want["csc_pos"], cp) and np.array_equal(want["csr_pos"], rp)
    v = np.concatenate([_stored(A2), _stored(G2)])
    # the column factor of every entry, as the first model shows it: sqrt(2)/2 on off-diagonal PSD columns, 1 elsewhere
    v0 = np.concatenate([_stored(pr.A), _stored(pr.G)])
    assert np.all(v0 != 0.0)
    cte = np.sqrt(2.0) / 2.0
    offcol = base["csc_val"][cp] != v0
    assert np.array_equal(base["csc_val"][cp], np.where(offcol, v0 * cte, v0))
    got = dict(csc_val_orig=np.zeros(base["nnz"]), csr_val_orig=np.zeros(base["nnz"]), csc_val=np.zeros(base["nnz"]),
               csr_val=np.zeros(base["nnz"]))
    got["csc_val_orig"][cp] = v
    got["csr_val_orig"][rp] = v
    got["csc_val"][cp] = np.where(offcol, v * cte, v)
    got["csr_val"][rp] = np.where(offcol, v * cte, v)
    for k, a in got.items():
        assert np.array_equal(a, want[k]), k
    order, od = _solver_order(pr), _offdiag_in_solver_order(pr)
    assert np.array_equal(want["c_orig"], c2[order])
    assert np.array_equal(want["c"], np.where(od, c2[order] * cte, c2[order]))
    assert np.array_equal(want["bh"], np.concatenate([pr2.b, pr2.h]))
    # the norms in prepare()'s order: one running sum over the caller's c, one over the scaled values in CSC order
    assert want["norm_c"] == float(np.sqrt(np.cumsum(c2 * c2)[-1]))
    assert want["frob"] == float(np.sqrt(np.cumsum(want["csc_val"] ** 2)[-1]))
