"""k_factor_residual alone (proxsdp_hip_factor_residual), in exact arithmetic.

V has entries in {-2..2}, lambda in {1, 2, 3}, X = V diag(lambda) V' is formed in int64 and handed over as the packed
upper triangle.  Every product, every partial sum of the MFMA chain and every sum of squares is an integer below 2^53
(asserted in the fixture), so the kernel's results are exact whatever its summation order: the assertions are `==`.
Sides 1, 2, 15, 16, 17, 63, 64, 65, 129 straddle the MFMA's 16 rows and the 64 x 64 tile (129: a 3 x 3 block triangle,
six workgroups, the XCD-interleaved tile order); ranks 0, 1, 3, 4, 5, 15, 16, 17, 33 the MFMA's k = 4 and the staged chunk
of 16 (33: three chunks, both LDS buffers reused)."""
import functools

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

SIDES = (1, 2, 15, 16, 17, 63, 64, 65, 129)
RANKS = (0, 1, 3, 4, 5, 15, 16, 17, 33)
PERTURBED_RANKS = (0, 4, 17)
D = 3


def _tri(n):
    jj = np.repeat(np.arange(n), np.arange(1, n + 1))
    ii = np.concatenate([np.arange(j + 1) for j in range(n)])
    return ii, jj


@functools.lru_cache(maxsize=None)
def case(n, r):
    """(packed int64, V int64 n x r, lambda int64, xnorm2 int) -- computed once, never modified by a test"""
    rng = np.random.default_rng(1000 * n + r)
    V = rng.integers(-2, 3, size=(n, r)).astype(np.int64)
    lam = rng.integers(1, 4, size=r).astype(np.int64)
    X = (V * lam) @ V.T
    assert np.array_equal(X, X.T)
    assert np.abs(X).max(initial=0) <= 12 * r                      # |entry| <= r * 3 * 2 * 2: <= 396 at r = 33
    xnorm2 = int((X * X).sum())
    assert xnorm2 < 3e9                                            # 129^2 * 396^2 = 2.6e9
    # largest value any accumulation can reach: squares of (|entry| + D), weight 2, all n^2 of them -- far below 2^53
    assert 2 * n * n * (12 * r + D) ** 2 < 2 ** 53
    ii, jj = _tri(n)
    packed = X[ii, jj]
    for a in (V, lam, packed):
        a.setflags(write=False)
    return packed, V, lam, xnorm2


def positions(n):
    """(0,0), (n-1,n-1), (0,n-1) and both sides of the tile edge where n allows"""
    pos = {(0, 0), (n - 1, n - 1), (0, n - 1)}
    for i, j in ((63, 63), (63, 64), (64, 64)):
        if j < n:
            pos.add((i, j))
    return sorted(pos)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIDES)
def test_residual_of_exact_factors_is_zero_and_the_norm_is_the_integer(n):
    for r in RANKS:
        packed, V, lam, xnorm2 = case(n, r)
        r2, x2 = B.factor_residual(packed.astype(float), n, V.astype(float), lam.astype(float))
        print(f"n={n} r={r}: resid2={r2!r} xnorm2={x2!r} (expected 0, {xnorm2})")
        if r == 0:
            assert xnorm2 == 0
        assert r2 == 0.0 and x2 == float(xnorm2), (n, r)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIDES)
def test_one_perturbed_entry_is_counted_once_on_the_diagonal_and_twice_off_it(n):
    for r in PERTURBED_RANKS:
        packed, V, lam, xnorm2 = case(n, r)
        Xd = {}
        for (i, j) in positions(n):
            x = packed.astype(float)
            q = j * (j + 1) // 2 + i
            x[q] += D
            w = 1 if i == j else 2
            r2, x2 = B.factor_residual(x, n, V.astype(float), lam.astype(float))
            exp_x2 = xnorm2 + w * (2 * D * int(packed[q]) + D * D)
            print(f"n={n} r={r} ({i},{j}): resid2={r2!r} (expected {w * D * D}) xnorm2={x2!r} (expected {exp_x2})")
            Xd[(i, j)] = (r2, x2, w * D * D, exp_x2)
        for (i, j), (r2, x2, e2, ex2) in Xd.items():
            assert r2 == float(e2) and x2 == float(ex2), (n, r, i, j)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIDES)
def test_padding_rows_of_v_are_never_read_into_a_sum(n):
    """ldv = n + 7 with NaN below row n: one NaN in any sum would make the result NaN"""
    for r in RANKS[1:]:
        packed, V, lam, xnorm2 = case(n, r)
        Vp = np.full((n + 7, r), np.nan)
        Vp[:n] = V
        r2, x2 = B.factor_residual(packed.astype(float), n, Vp, lam.astype(float))
        assert r2 == 0.0 and x2 == float(xnorm2), (n, r, r2, x2)
        x = packed.astype(float)
        x[-1] += D                                                 # (n-1, n-1): the entry next to the padding
        r2, x2 = B.factor_residual(x, n, Vp, lam.astype(float))
        assert r2 == float(D * D), (n, r, r2)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIDES)
def test_rank_zero_gives_the_norm_of_the_block(n):
    """r = 0 with X != 0: no factor is dereferenced (V, lam are NULL) and resid2 == xnorm2"""
    packed, V, lam, xnorm2 = case(n, 5)
    r2, x2 = B.factor_residual(packed.astype(float), n, np.zeros((n, 0)), np.zeros(0))
    assert r2 == float(xnorm2) and x2 == float(xnorm2)
    # the factors in the wrong scale: resid2 = ||X - 2 X||^2 = xnorm2, an exact integer again
    r2, x2 = B.factor_residual(packed.astype(float), n, V.astype(float), 2.0 * lam)
    assert r2 == float(xnorm2) and x2 == float(xnorm2)


@pytest.mark.gpu
def test_the_block_is_not_modified_and_the_result_repeats():
    n, r = 129, 33
    packed, V, lam, xnorm2 = case(n, r)
    x = packed.astype(float)
    x[5] += D
    keep = x.copy()
    a = B.factor_residual(x, n, V.astype(float), lam.astype(float))
    b = B.factor_residual(x, n, V.astype(float), lam.astype(float), repeat=3)
    assert np.array_equal(x, keep)
    assert a == b[:2] and b[2] > 0.0
