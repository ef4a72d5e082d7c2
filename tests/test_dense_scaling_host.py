"""Equilibration with a dense A, the part that needs no GPU: equilibrate! restated on the row sums of squares alone
(proxsdp_host_equilibrate_rowsums -- what the dense entry runs after its one device pass) against the oracle's
equilibrate on the whole matrix, and the two stats counters taken from the last reserved slots."""
import ctypes

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

from dense_scaling_cases import full_matrix, inst_a, inst_b, inst_c, oracle_scaling

CASES = {"A": inst_a, "B": inst_b, "C": inst_c}


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(b)))


# With the aliasing and bound rows present (A) the reference's iteration is chaotic: a 1e-15 relative perturbation of
# the data moves E by 12 % on the oracle alone.  No restatement can be pinned there, so A is compared without it only.
@pytest.mark.parametrize("name,aliasing", [("A", 0), ("B", 0), ("C", 0), ("B", 1), ("C", 1)])
def test_rowsum_equilibration_matches_oracle(name, aliasing):
    pr = CASES[name]()
    M = full_matrix(pr)
    Eo, Do = oracle_scaling(pr, aliasing)
    assert np.ptp(Do) == 0.0                                  # D is a multiple of the identity (equilibration.jl:56-58)
    o = B.default_options()
    o.equilibration_reference_aliasing = aliasing
    E, d = B.host_equilibrate_rowsums((M * M).sum(axis=1), M.shape[1], o)
    eE, eD = _rel(E, Eo), abs(d - Do[0]) / Do[0]
    print(f"{name} aliasing={aliasing}: rel err E {eE:.3e}, D {eD:.3e}")
    # the two differ in summation order only (measured 3e-11 in E): 1e-9 leaves 30x
    assert eE <= 1e-9 and eD <= 1e-9


def test_rowsum_equilibration_rejects_bad_arguments():
    with pytest.raises(B.ProxSDPHipError):
        B.host_equilibrate_rowsums(np.zeros(0), 5)
    with pytest.raises(B.ProxSDPHipError):
        B.host_equilibrate_rowsums(np.ones(3), 0)


def test_dense_scaling_stats_took_the_last_reserved_slots():
    names = [f[0] for f in B.Stats._fields_]
    assert names[-3:] == ["reserved_s", "dense_setup_passes", "dense_sigma_steps"]
    assert B.Stats.reserved_s.offset == B.Stats.wide_krylov_projections.offset + 8
    assert B.Stats.dense_setup_passes.offset == B.Stats.reserved_s.offset + 32
    assert ctypes.sizeof(B.Stats) == B.Stats.dense_sigma_steps.offset + 8
    assert B.lib().proxsdp_hip_abi_version() == 10
    assert {"proxsdp_hip_dense_scaling", "proxsdp_host_equilibrate_rowsums"} <= set(B.header_symbols())
