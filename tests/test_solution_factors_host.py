"""CPU-only tests of the factored solve's boundary (proxsdp_hip_solve_factored, proxsdp_psd_factors,
proxsdp_hip_factor_residual): the ctypes structure and the Julia shim list the header's members in order, the new
functions are exported under an unchanged ABI version, and every malformed proxsdp_psd_factors is rejected with
PROXSDP_E_INVALID on the host -- before a solver, and with it a device, exists (this machine has none: a call that got as
far as the device would come back with PROXSDP_E_HIP instead)."""
import ctypes as C
import re

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

from kat_problems import sdp_wiki
from test_host_abi import _c_struct_fields

NEW_FUNCTIONS = ("proxsdp_hip_solve_factored", "proxsdp_hip_factor_residual", "proxsdp_hip_factor_residual_kernel")


def test_factor_struct_mirrors_the_header_field_by_field():
    header = B.HEADER_PATH.read_text()
    cf = _c_struct_fields(header, "proxsdp_psd_factors")
    assert [f for f, _ in B.PsdFactors._fields_] == cf
    assert C.sizeof(B.PsdFactors) == 8 * len(cf)                     # twelve 8-byte members, no padding
    jl = (B.HEADER_PATH.parent.parent / "julia" / "ProxSDPHip.jl").read_text()
    body = re.search(r"struct PsdFactors\b.*?\n(.*?)\nend", jl, re.S).group(1)
    jf = [re.match(r"\s*(\w+)::", ln).group(1) for ln in body.splitlines() if re.match(r"\s*\w+::", ln)]
    assert jf == cf
    for name, value in (("PROXSDP_FACTOR_NONE", B.FACTOR_NONE), ("PROXSDP_FACTOR_RITZ", B.FACTOR_RITZ),
                        ("PROXSDP_FACTOR_EIG", B.FACTOR_EIG)):
        assert int(re.search(r"#define %s\s+(\d+)" % name, header).group(1)) == value


def test_new_functions_are_exported_and_the_abi_version_stays():
    L = B.lib()
    names = set(B.header_symbols())
    for f in NEW_FUNCTIONS:
        assert f in names, f"{f} is not declared in include/proxsdp_hip.h"
        assert hasattr(L, f), f"{f} is not exported"
    assert L.proxsdp_hip_abi_version() == 10
    jl = (B.HEADER_PATH.parent.parent / "julia" / "ProxSDPHip.jl").read_text()
    assert ":proxsdp_hip_solve_factored" in jl


def _call(prob, mutate):
    """proxsdp_hip_solve_factored on `prob` with a well-formed proxsdp_psd_factors that `mutate` then damages"""
    L = B.lib()
    M = B._Marshalled(prob)
    o = B.default_options()
    R = B.Result()
    F, arr = B._factors_struct(B.psd_sides(prob), True)
    keep = mutate(F, arr, M)
    rc = L.proxsdp_hip_solve_factored(C.byref(M.P), C.byref(o), C.byref(R), C.byref(F) if F is not None and keep is not False else None)
    return rc, L.proxsdp_hip_last_error().decode()


def _set(field, value):
    def m(F, arr, M):
        setattr(F, field, value)
    return m


def _short_vec(F, arr, M):
    arr["vec_ptr"][1] = 3 * 3 - 1                                    # side 3, cap 3: one double short


def _short_val(F, arr, M):
    arr["val_ptr"][1] = 2


def _negative_cap(F, arr, M):
    arr["cap"][0] = -1


INVALID = {
    "n_psd_mismatch": _set("n_psd", 2),
    "struct_size": _set("struct_size", 8),
    "null_cap": _set("cap", None),
    "null_vec_ptr": _set("vec_ptr", None),
    "null_val_ptr": _set("val_ptr", None),
    "null_vectors": _set("vectors", None),
    "null_values": _set("values", None),
    "null_rank": _set("rank", None),
    "null_rank_found": _set("rank_found", None),
    "null_source": _set("source", None),
    "null_resid": _set("resid", None),
    "null_xnorm": _set("xnorm", None),
    "vec_span_too_small": _short_vec,
    "val_span_too_small": _short_val,
    "negative_cap": _negative_cap,
    "null_struct": lambda F, arr, M: False,
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_malformed_factors_are_rejected_before_touching_the_device(case):
    rc, msg = _call(sdp_wiki(False), INVALID[case])
    assert rc == -1, (case, rc, msg)                                 # PROXSDP_E_INVALID, not PROXSDP_E_HIP
    assert msg


def test_a_shard_is_refused_on_the_host():
    """PROXSDP_E_UNSUPP for a problem that is a shard, decided before the device is touched as well"""
    def shard(F, arr, M):
        cb = B.REDUCE_FN(lambda ctx, ps, ns, pm, nm: 0)
        M.keep.append(cb)
        M.P.reduce_fn = C.cast(cb, C.c_void_p)
    rc, msg = _call(sdp_wiki(False), shard)
    assert rc == -4 and "shard" in msg

    def coupled(F, arr, M):
        M.P.n_coupling = 1
    assert _call(sdp_wiki(False), coupled)[0] == -4


def test_well_formed_factors_reach_the_device():
    """the control of the cases above: the unharmed struct passes the host checks (without a GPU the call then fails
    with PROXSDP_E_HIP, with one it solves)"""
    rc, msg = _call(sdp_wiki(False), lambda F, arr, M: None)
    assert rc == (0 if B.device_count() > 0 else -2), msg


def test_binding_caps_and_offsets():
    F, arr = B._factors_struct([3, 1, 5], {0: 2, 2: 9})
    assert list(arr["cap"]) == [2, 0, 5]                             # capped at the side; an unnamed cone gets nothing
    assert list(arr["vec_ptr"]) == [0, 6, 6, 31] and list(arr["val_ptr"]) == [0, 2, 2, 7]
    assert F.struct_size == C.sizeof(B.PsdFactors) and F.n_psd == 3
    with pytest.raises(ValueError):
        B._factors_struct([3], {1: 1})
    with pytest.raises(ValueError):
        B.solve(sdp_wiki(False), factors=True, capture_iteration=3)
    assert B.psd_sides(sdp_wiki(False)) == [3]
    out = B._factors_list([2], dict(rank=np.array([1]), rank_found=np.array([2]), source=np.array([1], dtype=np.int32),
                                    resid=np.array([0.5]), xnorm=np.array([2.0]), cap=np.array([1]),
                                    vec_ptr=np.array([0, 2]), val_ptr=np.array([0, 1]),
                                    vectors=np.array([0.6, 0.8]), values=np.array([3.0])))
    vals, vecs, info = out[0]
    assert vals.tolist() == [3.0] and vecs.shape == (2, 1) and vecs[:, 0].tolist() == [0.6, 0.8]
    assert info["source_name"] == "RITZ" and info["rank_found"] == 2 and info["resid"] == 0.5
