"""CPU checks of the fixtures and references of the sign-product tests (sign_product_cases.py): the exact family cannot leave
53 bits (integer arithmetic), its operand pairs are what their names say, the expected matrices carry the written-set rules,
the fused-residual layouts plant what they claim, the rounded bound already holds for a plain fp64 NumPy evaluation, and the
binding exposes the entries."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import sign_product_cases as S

ALL_SIDES = sorted({n for t in S.SIDES.values() for n in t})


def test_binding_exposes_the_entries_and_mirrors_the_struct():
    assert B.lib().proxsdp_hip_abi_version() == 10
    assert {"proxsdp_hip_sym_product", "proxsdp_hip_sign_unpack"} <= set(B.header_symbols())
    assert hasattr(B.lib(), "proxsdp_hip_sym_product") and hasattr(B.lib(), "proxsdp_hip_sign_unpack")
    assert callable(B.sym_product) and callable(B.sign_unpack)
    import test_host_abi as H
    cf = H._c_struct_fields(_named(B.HEADER_PATH.read_text()), "proxsdp_sym_product")
    assert [f for f, _ in B.SymProductIO._fields_] == cf
    assert B.SYM_SENTINEL == S.SENTINEL


def _named(header):
    """the header declares `typedef struct { .. } proxsdp_sym_product;`: give the struct its name for the field parser"""
    import re
    m = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} proxsdp_sym_product;", header, re.S)
    return "typedef struct proxsdp_sym_product {" + m.group(1) + "} proxsdp_sym_product;"


def test_without_a_device_the_entries_fail_loudly():
    if B.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(B.ProxSDPHipError) as e:
        B.sym_product(np.eye(3), np.eye(3), tile=64)
    assert e.value.code == -2
    with pytest.raises(B.ProxSDPHipError):
        B.sign_unpack(np.ones(6), 3)


def test_shapes_reach_every_mechanism():
    # 64-tiles: nt = 1 is two pipeline groups (ngroups = 2 nt); nt = 4, 5, 6 are 10, 15, 21 tiles in grids of 16, 16, 24
    assert [S.tiles_per_side(n, 64) for n in (1, 63, 64)] == [1, 1, 1] and S.tiles_per_side(65, 64) == 2
    assert [(S.tiles_per_side(n, 64), S.grid_of(n, 64)) for n in (200, 257, 330)] == [(4, 16), (5, 16), (6, 24)]
    for n in (200, 257, 330):
        slots = S.slot_tiles(n, 64)
        real = [s for s in slots if s is not None]
        nt = S.tiles_per_side(n, 64)
        assert len(real) == nt * (nt + 1) // 2 == len(set(real)) and None in slots          # padding workgroups exist
        assert slots[:8] != sorted(real)[:8]                                                  # interleaved, not sequential
    # 32-tiles: nsteps = ld / 64 = 1 at ld = 64 (the branch without a pipeline), 2 and 4 beyond
    assert {S.ld_of(n) // 64 for n in S.SIDES[32]} == {1, 2, 4}
    # 48-tiles: ngroups = ld / 64 = 1, 2, 3, 4 among the sides the solver's rule admits; the rule refuses 49, 100, 250
    ok = [n for n in S.SIDES[48] if S.tile48_fits(n)]
    assert ok == [47, 48, 96, 144, 145, 192, 240] and {S.ld_of(n) // 64 for n in ok} == {1, 2, 3, 4}
    assert [n for n in S.SIDES[48] if not S.tile48_fits(n)] == [49, 100, 250]
    assert any(48 * S.tiles_per_side(n, 48) < S.ld_of(n) for n in ok)                         # rows the 48-tiles never write
    assert any(n < 48 * S.tiles_per_side(n, 48) for n in ok)                                  # padding inside the tiles
    assert max(S.ROUNDED_SIDES) <= 130 and all(S.tile48_fits(n) for n in S.ROUNDED_SIDES)


@pytest.mark.parametrize("n", ALL_SIDES)
def test_exact_family_stays_inside_53_bits(n):
    for cs in S.exact_cases(n):
        units, U = S.exact_proof(cs)
        assert isinstance(units, int) and units < 2 ** 53, (n, cs["name"], units.bit_length())
        for M in (cs["Pi"], cs["Qi"]) + ((cs["Yi"],) if cs["Yi"] is not None else ()):
            assert M.dtype == np.int64 and np.array_equal(M, M.T)
            assert int(np.abs(M).max()) < 2 ** 53
        for c in S.coefficients(cs) + (cs["dsc"] or ()):
            fr = Fraction(c)
            assert fr.denominator & (fr.denominator - 1) == 0 and abs(fr.numerator) <= 8      # small integers, powers of two


def test_width_bound_of_the_largest_case():
    """From the widths alone, for the largest padded side: 20-bit operands, K = 384 terms, |kc| = 1 and the Y term."""
    K = max(S.ld_of(n) for n in ALL_SIDES)
    assert K == 384
    M = 2 ** 20 - 1
    cs = [c for c in S.exact_cases(2) if c["name"] == "generic"][0]
    ka, kb, kc = (Fraction(c) for c in S.coefficients(cs))
    assert (ka, kb, kc) == (-2, 2, 1)
    # finest unit: 2^-(20 + 7) of the product; Y lives on 2^-9, ka on 1
    worst = K * M * M + abs(kb) * M * 2 ** (27 - 9) + abs(ka) * 2 ** 27
    assert worst < 2 ** 53 and worst.numerator.bit_length() == 49
    assert S.exact_proof([c for c in S.exact_cases(330) if c["name"] == "generic"][0])[0] <= worst


@pytest.mark.parametrize("n", [2, 65, 200])
def test_float_evaluation_of_the_exact_reference_is_the_rational_value(n):
    """expected_full evaluates the epilogue in fp64; with every term inside 53 bits that IS the rational value"""
    for cs in S.exact_cases(n):
        ka, kb, kc = (Fraction(c) for c in S.coefficients(cs))
        PQ = cs["Pi"].astype(object) @ cs["Qi"].astype(object)                  # Python integers
        E = S.expected_full(cs)
        for i, j in [(0, 0), (0, n - 1), (n - 1, 0), (n // 2, n // 3), (n - 1, n - 1)]:
            v = kc * Fraction(int(PQ[i, j]), 2 ** (cs["bp"] + cs["bq"]))
            if cs["epilogue"] == "poly":
                v += kb * Fraction(int(cs["Yi"][i, j]), 2 ** cs["by"]) + (ka if i == j else 0)
            assert Fraction(float(E[i, j])) == v, (cs["name"], i, j)


@pytest.mark.parametrize("n", [31, 65, 200, 330])
def test_operand_kinds_are_what_they_claim(n):
    cases = {c["name"]: c for c in S.exact_cases(n)}
    for nm in ("AA", "YY", "XQ"):
        P, Q = cases[nm]["Pi"], cases[nm]["Qi"]
        assert np.array_equal(P @ Q, Q @ P), nm                                 # commuting: the full product is symmetric
    assert cases["YY"]["Yi"] is cases["YY"]["Pi"]                               # Y Y with Y as the epilogue operand
    g = cases["generic"]
    PQ = g["Pi"] @ g["Qi"]
    assert not np.array_equal(g["Pi"], g["Qi"])
    assert np.count_nonzero(PQ != PQ.T) > 0.9 * n * (n - 1)                     # a transposed operand map shows nearly everywhere
    E = S.expected_T(g, 64)[:n, :n]
    F = S.expected_full(g)
    assert np.array_equal(np.triu(E), np.triu(F)) and np.array_equal(E, E.T) and not np.array_equal(np.tril(E), np.tril(F))
    L = cases["lowrank"]
    PQ = L["Pi"] @ L["Qi"]
    nzv = np.abs(PQ[PQ != 0])
    assert np.count_nonzero(PQ == 0) >= n and nzv.min() <= 7 and nzv.max() >= 2 ** 30           # exact zeros, entries 2^30 apart
    assert np.linalg.matrix_rank(L["Pi"].astype(float)) <= 2 and np.linalg.matrix_rank(L["Qi"].astype(float)) <= 2
    # every aligned k-step (4 k) and every pipeline group of the kernels (8 k for 64-tiles, 16 k for 32- and 48-tiles) carries a
    # non-zero contribution to the product: dropping or repeating one changes the result
    for step in (4, 8, 16):
        for k0 in range(0, n, step):
            blk = L["Pi"][:, k0:k0 + step] @ L["Qi"][k0:k0 + step, :]
            assert np.any(blk != 0), (step, k0)
    assert np.any((L["Pi"] != 0).all(axis=0))                                   # (u has no zero: a term at every k)


@pytest.mark.parametrize("tile,n", [(t, n) for t in (64, 32, 48) for n in S.SIDES[t] if t != 48 or S.tile48_fits(n)])
def test_expected_matrices_carry_the_written_set_rules(tile, n):
    ld, w = S.ld_of(n), S.written_side(n, tile)
    assert w == (ld if tile != 48 else 48 * (-(-n // 48))) and n <= w <= ld
    for cs in S.exact_cases(n):
        T = S.expected_T(cs, tile)
        assert T.shape == (ld, ld)
        out = np.ones((ld, ld), dtype=bool)
        out[:w, :w] = False
        assert np.all(T[out] == S.SENTINEL) and not np.any(T[~out] == S.SENTINEL)
        pad = T[:w, :w].copy()
        pad[:n, :n] = 0.0
        if cs["epilogue"] == "plain":
            assert not pad.any()
        else:
            ka = S.coefficients(cs)[0]
            assert ka != 0 and np.array_equal(pad, np.diag(np.r_[np.zeros(n), np.full(w - n, ka)]))
        part = S.expected_part(cs, tile)
        slots = S.slot_tiles(n, tile)
        assert len(part) == S.grid_of(n, tile) == len(slots)
        assert all(part[b] == 0.0 for b, s in enumerate(slots) if s is None)
        fro, U = S.fro_units(cs, tile)
        if cs["name"] in ("AA", "XQ"):
            # plain, narrow operands: the Frobenius partials are exact in any order
            assert fro < 2 ** 53
            assert Fraction(float(part.sum())) == Fraction(fro, 4 ** U) == Fraction(float(np.sum(T[:n, :n] ** 2)))
        else:
            assert abs(float(part.sum()) * 4.0 ** U / fro - 1) < 1e-12


@pytest.mark.parametrize("n", S.FINAL_SIDES)
def test_final_fixtures(n):
    N = n * (n + 1) // 2
    gi, gj = S.packed_index(n)
    assert len(gi) == N and np.array_equal(gj * (gj + 1) // 2 + gi, np.arange(N))
    for variant in ("plain", "diag", "lastcol", "empty", "clamp"):
        cs = S.final_case(n, variant)
        units, U = S.exact_proof(cs, final=True)
        assert units < 2 ** 53
        assert not np.array_equal(cs["Pi"] @ cs["Qi"], cs["Qi"] @ cs["Pi"])
        # x+ = fl(c v) with v exact: one rounding, checked against the rational value
        m0 = Fraction(S.coefficients(cs)[2])
        PQ = cs["Pi"].astype(object) @ cs["Qi"].astype(object)
        for k in (0, N // 2, N - 1):
            v = Fraction(int(cs["Pi"][gi[k], gj[k]]), 2 ** cs["bp"]) + m0 * Fraction(int(PQ[gi[k], gj[k]]), 2 ** (cs["bp"] + cs["bq"]))
            c = 0.5 if gi[k] == gj[k] else 0.5 * S.SQRT2
            assert cs["xp"][k] == c * float(v) and Fraction(float(v)) == v
        assert expected_trace(cs) == cs["trace_q"]
        if variant == "plain":
            continue
        assert cs["mask_off"] % 32 != 0
        words = cs["mask"][cs["mask_off"] // 32:(cs["mask_off"] + N + 31) // 32]
        if variant != "empty" or n > S.TILE:
            assert np.any((words != 0) & (words != 0xFFFFFFFF))                 # on and off bits in the same word
        on = cs["on"]
        assert all(bool((cs["mask"][(cs["mask_off"] + k) >> 5] >> ((cs["mask_off"] + k) & 31)) & 1) == bool(on[k])
                   for k in range(0, N, max(1, N // 97)))
        diff = np.abs(cs["xp"] - cs["xold"])
        r = cs["respart"]
        assert r.shape == (2, S.grid_of(n, 64))
        if variant in ("diag", "lastcol"):
            k = cs["planted"]
            assert (gi[k] == gj[k]) if (variant == "diag" or n == 1) else (gj[k] == n - 1 and gi[k] < gj[k])
            assert not on[k] and diff[k] == r[0].max() == 64.0 and diff[~on].max() == 64.0
            near = [q for q in (k - 1, k + 1) if 0 <= q < N]
            assert near and all(on[q] and diff[q] > 1000 for q in near)          # one entry off and the maximum is wrong
        if variant == "empty":
            sel = cs["empty_sel"]
            assert sel.any() and on[sel].all()
            tiles = {(int(a), int(b)) for a, b in zip(gi[sel] // 64, gj[sel] // 64)}
            for b, ij in enumerate(S.slot_tiles(n, 64)):
                if ij in tiles:
                    assert r[0, b] == 0.0 and r[1, b] == 0.0
            if n > S.TILE:
                assert r[0].max() > 0
        if variant == "clamp":
            last = gj == n - 1
            assert n % S.TILE != 0 or n == 64                                    # (n = 64 has no clamped lane: kept as the control)
            assert not on[last].any() and np.abs(cs["xold"][last]).max() >= 1000 * diff.max()


def expected_trace(cs):
    return float(S.expected_trace_part(cs).sum())


@pytest.mark.parametrize("n", S.ROUNDED_SIDES)
def test_rounded_bound_holds_for_plain_numpy(n):
    assert np.finfo(np.longdouble).nmant >= 63
    A, xp = S.rounded_matrix(n)
    assert np.array_equal(A, A.T) and np.all(np.frexp(A)[0] * 2.0 ** 53 % 2 ** 20 != 0)         # full mantissas
    sc = S.host_scalars(A)
    assert sc[4] >= np.abs(np.linalg.eigvalsh(A)).max()
    worst = 0.0
    for cs in S.rounded_cases(A, sc):
        assert np.array_equal(cs["P"], cs["P"].T) and np.array_equal(cs["Q"], cs["Q"].T)
        ref, bound = S.rounded_reference(cs)
        err = np.abs((S.rounded_numpy(cs).astype(np.longdouble) - ref).astype(np.float64))
        ratio = float((err / bound).max())
        print(f"n={n} {cs['name']}: NumPy fp64 error / bound = {ratio:.3f}")
        assert np.all(err <= bound), (n, cs["name"], ratio)
        worst = max(worst, ratio)
    assert 0 < worst < 1
    rows, cubic = S.sign_table()
    assert cubic and len(rows) == 19 and rows[0][0] == 4.256725463981158 and rows[8][2] == 9.378715974021034


@pytest.mark.parametrize("n", S.UNPACK_SIDES)
def test_unpack_reference(n):
    A, xp = S.rounded_matrix(n)
    R, f2, rel = S.unpack_reference(xp, n)
    assert np.array_equal(R, R.T) and np.array_equal(np.diag(R), np.diag(A))
    assert np.all(np.abs(R - A) <= 4 * 2.0 ** -53 * np.abs(A))                  # fl(fl(sqrt2 a) inv_sqrt2): two roundings, two rounded constants
    assert abs(math.fsum((R * R).ravel()) / float(f2) - 1) <= rel + 2.0 ** -52
