"""CPU checks of the per-cycle Lanczos tests (lanczos_cycle_cases.py): every case restarts as often as its GPU test asks for,
the plain reference itself stays below 32 x 2^-52 sqrt(K) in every quantity (no bound of the GPU test is vacuous), deliberately
wrong variants of the reference fail the GPU test's own rule, the binding mirrors the header's struct and the entry refuses
invalid arguments before it touches a device."""
import ctypes
import math
import re

import numpy as np
import pytest

from oracle import eig as oeig
from proxsdp_jl_amd import binding as B

import lanczos_cycle_cases as L


def _distinct(cases):
    seen, out = set(), []
    for cs in cases:
        key = (cs["n"], cs["nev"], cs["kd"], cs["opts"].get("eigsolver", 2))
        if key not in seen:
            seen.add(key)
            out.append(cs)
    return out


RUNS = _distinct(L.CASES)


def test_long_double_is_the_80_bit_format():
    assert np.finfo(L.LD).eps < 1e-18


def test_the_table_reaches_every_engine_and_path():
    assert {c["engine"] for c in L.CASES} == {"step", "block1", "wide"}
    assert all(c["kd"] == max(2 * c["nev"] + 1, c["opts"]["eigsolver_min_lanczos"]) for c in L.CASES)
    assert all(c["cycles"] == (3 if c["oracle_cycles"] is None or c["oracle_cycles"] >= 3 else 2) for c in L.CASES)
    kds = sorted({c["kd"] for c in L.CASES})
    assert kds[0] <= 16 and any(64 < k <= 128 for k in kds) and any(128 < k <= 192 for k in kds) and 255 in kds and 261 in kds
    assert any(c["n"] > 4096 for c in L.CASES) and any(c["n"] % 64 == 1 for c in L.CASES)
    assert any((3 * c["kd"]) // 5 >= 132 and c["engine"] == "step" for c in L.CASES)      # keep >= 132: the third loop of f'h
    for flag in ("split", "merge_on_device", "speculated"):
        assert any(flag in c["flags"] for c in L.CASES)


@pytest.mark.parametrize("cs", RUNS, ids=[c["id"] for c in RUNS])
def test_oracle_restarts_often_enough_and_the_reference_is_accurate(cs):
    """the CPU side of the GPU test's condition (no case passes with its restarted cycle missing), and the reference's own
    R1 - R3.  dsaupd's rule (eigsolver = 1) has no cycle count in the oracle (SciPy's ARPACK restarts implicitly): the
    reference run with the library's restatement of the rule stands in for it."""
    n, nev, kd = cs["n"], cs["nev"], cs["kd"]
    A, _, normA = L.matrix(n, nev)
    arpack = cs["opts"].get("eigsolver", 2) == 1
    if not arpack:
        numiter = oeig.krylovkit_eigsolve(lambda v: A @ v, oeig.start_vector(n), nev, kd, 100, L.TOL)[3]
        assert numiter >= cs["cycles"], (numiter, cs["cycles"])
        assert abs(numiter - cs["oracle_cycles"]) <= 1                    # (the table's counts, up to the seed of Q)
    run, early = L.reference_run(A, L.start(n), nev, kd, cs["cycles"], tol=1e-10 if arpack else L.TOL, arpack=arpack)
    assert not early and len(run) == cs["cycles"]
    reuse = None
    for c, cyc in enumerate(run):
        q, reuse = L.quantities(A, normA, cyc, reuse)
        assert (cyc["kfirst"] == 0) == (c == 0) and q["beta_min"] > 0.0
        for name in L.QUANTITIES:
            assert q[name] <= L.HOST_BOUND * math.sqrt(cyc["K"]), (c, name, q[name])


@pytest.mark.parametrize("variant", ["one_pass", "no_fh", "alpha_1e13"])
@pytest.mark.parametrize("n,nev,kd", [(129, 14, 30), (300, 64, 130)])
def test_wrong_variants_fail_the_rule_of_the_gpu_test(variant, n, nev, kd):
    """cycles of a wrong variant, judged as the GPU test judges a kernel's -- against the plain reference run from the same
    inputs, with the same margin and floor.  The rule judges a cycle GIVEN its inputs: once a basis is spoilt, the reference
    run from it is no better, so a lasting defect shows in the first cycle that commits it (which is enough to fail the
    run), a defect of the coefficients alone in every cycle.  The second pass left out: the first cycle, by R2 and beta; the
    f'h row left out with a local second pass: R2 in the first cycle, R1 in the first restarted one; alpha off by 1e-13:
    R3 in every cycle."""
    A, _, normA = L.matrix(n, nev)
    run, _ = L.reference_run(A, L.start(n), nev, kd, 3, variant=variant)
    flagged = []
    for c, cyc in enumerate(run):
        Vr, alr, ber = L.reference_cycle(A, cyc["V"], cyc["kfirst"], cyc["K"])
        qw, reuse = L.quantities(A, normA, cyc)
        qr, _ = L.quantities(A, normA, dict(cyc, V=Vr, alphas=alr, betas=ber), reuse)
        flagged.append({name for name in L.QUANTITIES if qw[name] > L.bound(qr[name])})
    if variant == "one_pass":
        assert {"r2", "r3_beta"} <= flagged[0], flagged
    elif variant == "no_fh":
        assert "r2" in flagged[0] and {"r1_own", "r1_all", "r2"} <= flagged[1], flagged
    else:
        assert all("r3_alpha" in fl for fl in flagged), flagged


def test_rank5_matrix_is_exact():
    A, packed, normA = L.rank5_matrix(130)
    assert np.array_equal(A, A.T) and np.linalg.matrix_rank(A) == 5
    assert np.array_equal(A * 16.0, np.round(A * 16.0))                   # sixteenths: every entry exact
    ev = np.sort(np.linalg.eigvalsh(A))[::-1]
    assert np.allclose(ev[:5], [9.0, 7.0, 5.0, 3.0, 2.0], atol=1e-13) and np.abs(ev[5:]).max() <= 1e-13
    # six plain Lanczos steps exhaust the Krylov space of the start vector
    V, al, be = L.reference_cycle(A, L.start(130)[:, None] * np.ones((1, 31)), 0, 6)
    assert be[5] <= L.TOL and np.all(be[:5] > 1e-3)


def _named(header, name):
    m = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + name + ";", header, re.S)
    return "typedef struct " + name + " {" + m.group(1) + "} " + name + ";"


def test_binding_exposes_the_entry_and_mirrors_the_struct():
    assert B.lib().proxsdp_hip_abi_version() == 10
    assert "proxsdp_hip_lanczos_cycles" in set(B.header_symbols()) and hasattr(B.lib(), "proxsdp_hip_lanczos_cycles")
    import test_host_abi as T
    header = B.HEADER_PATH.read_text()
    name = "proxsdp_lanczos_cycles"
    assert [f for f, _ in B.LanczosCyclesIO._fields_] == T._c_struct_fields(_named(header, name), name)
    # every member is 4 or 8 bytes wide and the 4-byte ones come in pairs: no padding, the size is the sum
    assert ctypes.sizeof(B.LanczosCyclesIO) == 8 + 4 * 6 + 8 * 3 + 8 + 8 * 6 + 4 * 4 == 128
    engines = {int(v): k.lower() for k, v in re.findall(r"#define PROXSDP_LZ_ENGINE_(\w+)\s+(\d+)", header)}
    assert engines == B.LZ_ENGINES == {0: "step", 1: "block1", 2: "wide"}
    assert int(re.search(r"#define PROXSDP_LZ_INFO\s+(\d+)", header).group(1)) == B.LZ_INFO == 12


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """code -1 with or without a GPU; a valid call without one fails loudly with -2"""
    x = np.zeros(10 * 11 // 2)

    def refused(match, nev, max_cycles, **opts):
        o = B.default_options()
        for k, v in opts.items():
            B.set_option(o, k, v)
        with pytest.raises(B.ProxSDPHipError, match=match) as e:
            B.lanczos_cycles(x, 10, nev, max_cycles, options=o)
        assert e.value.code == -1

    refused("nev must be", 0, 2, eigsolver_min_lanczos=5)
    refused("nev must be", 11, 2)
    refused("max_cycles < 1", 2, 0, eigsolver_min_lanczos=5)
    refused("beyond the workspace", 2, 2, eigsolver_min_lanczos=512, lanczos_wide_krylov=1)
    refused("needs the wide workspace", 2, 2, eigsolver_min_lanczos=261)
    refused("another driver", 2, 2, eigsolver_min_lanczos=5, krylovkit_eager=1)
    big = np.zeros(300 * 301 // 2)
    with pytest.raises(B.ProxSDPHipError, match="needs the wide workspace") as e:
        B.lanczos_cycles(big, 300, 130, 2)                                 # krylovdim 261 without lanczos_wide_krylov
    assert e.value.code == -1
    if B.device_count() <= 0:
        o = B.default_options()
        B.set_option(o, "eigsolver_min_lanczos", 5)
        with pytest.raises(B.ProxSDPHipError) as e:
            B.lanczos_cycles(np.ones(55), 10, 2, 2, options=o)
        assert e.value.code == -2
