"""CPU checks of tests/small_block_cases.py: the references the GPU tests of the small-block projections are held to, the
layouts, and the NumPy restatement of the kernel's Jacobi (test_small_blocks.py runs the device side)."""
import numpy as np
import pytest

import small_block_cases as SC
from proxsdp_jl_amd import binding as B

LD = SC.LD
ALL_CASES = [c for d in range(SC.DEALS) for c in SC.deal(d) if c is not None]


def test_entry_is_declared_exported_and_bound():
    assert "proxsdp_hip_project_cones" in set(B.header_symbols())
    assert hasattr(B.lib(), "proxsdp_hip_project_cones") and callable(B.project_cones)
    assert B.BLOCK_CLASSES == ("1x1", "small-jacobi", "small-sign", "large")


def test_every_side_meets_every_spectrum():
    seen = {(c.n, c.kind) for c in ALL_CASES}
    assert seen == {(s, k) for s in SC.SIDES if s > 1 for k in SC.SPECTRA}
    # the three blocks of side 2 carry different data in every deal (the reorder test swaps two of them)
    for d in range(SC.DEALS):
        twos = [c for c in SC.deal(d) if c is not None and c.n == 2]
        assert len({c.kind for c in twos}) == 3
        sw = [c for c in SC.deal(d, swap=True) if c is not None and c.n == 2]
        assert sw[0] is twos[2] and sw[2] is twos[0] and sw[1] is twos[1]


def test_reference_error_is_below_1e_15_of_the_scale():
    """non-expansiveness: |ref - P(X64)|_F <= |X64 - Xld|_F + 2 |Q'Q - I|_F scale; at side 64 about sqrt(64) 2^-53"""
    worst = 0.0
    for c in ALL_CASES:
        if c.scale == 0.0:
            assert c.ref_err == 0.0 and not c.X64.any() and not c.ref.any()
            continue
        worst = max(worst, c.ref_err / c.scale)
        assert c.ref_err <= 1e-15 * c.scale, (c.kind, c.n, c.ref_err / c.scale)
    print(f"worst reference error bound: {worst:.3e} x scale")


def test_references_are_projections():
    """what a projection onto the PSD cone satisfies, checked in longdouble: ref is symmetric and PSD, X - ref is NSD and
    orthogonal to ref -- to the accuracy of the bound above"""
    for c in ALL_CASES:
        if c.scale == 0.0:
            continue
        X, R = c.X64.astype(LD), c.ref
        assert np.array_equal(R, R.T) and np.array_equal(c.X64, c.X64.T)
        tol = 4e-15 * c.scale * c.n
        assert np.linalg.eigvalsh(R.astype(np.float64)).min() >= -tol
        assert np.linalg.eigvalsh((X - R).astype(np.float64)).max() <= tol
        assert abs(float((R * (X - R)).sum())) <= tol * c.scale * c.n


def test_closed_form_and_scaled_cases():
    for n in (s for s in SC.SIDES if s > 1):
        c = SC.case("aI_bee", n, 0)
        top = -1.0 + n / 2.0
        assert np.array_equal(c.X64, -np.eye(n) + 0.5) and c.rank == c.npos == (1 if top > 0 else 0)
        assert np.allclose(c.ref.astype(np.float64), max(top, 0.0) / n, rtol=1e-15, atol=0)
        b = SC.case("decades", n, 0)
        for kind, f in (("tiny", SC.TINY), ("huge", SC.HUGE)):
            s = SC.case(kind, n, 0)
            assert np.array_equal(s.X64, b.X64 * f) and np.array_equal(s.ref, b.ref * LD(f)) and s.npos == b.npos
            assert np.array_equal(s.x, b.x * f) and s.s_ref == b.s_ref
        assert SC.case("tiny", n, 0).rank == 0 and float(np.abs(SC.case("tiny", n, 0).X64).max()) ** 2 == 0.0   # squares underflow
        with np.errstate(over="ignore"):
            assert np.isinf(np.square(np.abs(SC.case("huge", n, 0).X64).max()))                               # ... and overflow
        k = n // 3
        r = SC.case("repeated", n, 0)
        assert (r.rank, r.npos, r.nzero) == (k, k, n - 2 * k)
        dg = SC.case("diagonal", n, 0)
        assert not (dg.X64 - np.diag(np.diag(dg.X64))).any() and dg.degenerate and dg.s_ref == 0


def test_svec_round_trip_and_layouts():
    rng = np.random.default_rng(0)
    M = rng.standard_normal((7, 7)); M = M + M.T
    back = SC.smat_ld(SC.svec(M), 7).astype(np.float64)
    assert np.allclose(back, M, rtol=4e-16, atol=0)
    for layout, free in SC.LAYOUTS.items():
        offs, sides, (so, sl), fo, n = SC.block_table(free)
        assert offs[0] == 0 and all(offs[i + 1] == offs[i] + SC.packed_len(sides[i]) for i in range(len(offs) - 1))
        assert so == offs[-1] + SC.packed_len(sides[-1]) and fo == so + sl and n == fo + free
        assert (n > 65536) == (layout == "padded")          # the rank record's two routes
        x, cases = SC.vector(layout, 3)
        sent = SC.sentinel(n)
        assert np.array_equal(x[so:], sent[so:]) and np.isfinite(x).all() and len(np.unique(sent[so:so + 12])) == 12
        for o, s, c in zip(offs, sides, cases):
            assert (c is None) == (s == 1)
            if c is not None:
                assert np.array_equal(x[o:o + SC.packed_len(s)], c.x)
    xm, _ = SC.vector("mixed", 5)
    xp, _ = SC.vector("padded", 5)
    assert np.array_equal(xm, xp[:len(xm)])


def test_round_robin_schedule_covers_every_pair_once():
    for n in (2, 3, 5, 16, 17, 64):
        rounds = SC.round_robin(n)
        assert len(rounds) == n + (n & 1) - 1
        pairs = [pq for r in rounds for pq in r]
        assert sorted(pairs) == [(p, q) for p in range(n) for q in range(p + 1, n)]
        for r in rounds:
            flat = [i for pq in r for i in pq]
            assert len(set(flat)) == len(flat)              # disjoint within a round


@pytest.mark.parametrize("n", [2, 5, 17, 48, 64])
def test_restated_jacobi_converges_and_its_stall_rule_is_sound(n):
    """the restatement diagonalises (its own check, not the device's), its stall rule leaves within 1e-13 of the scale, and
    the bare rule "a sweep gained less than a factor of 10" would not: far from convergence it fires at once"""
    early = 0
    for kind in ("indefinite", "posdef", "decades", "repeated", "aI_bee"):
        c = SC.case(kind, n, 0)
        ratios, s, A, V = SC.restated_jacobi(c.X64)
        assert s == c.s_ref and 0 < s < 40 or c.degenerate
        lam = np.diag(A)
        proj = ((V * np.maximum(lam, 0.0)) @ V.T).astype(LD)
        assert float(np.abs(proj - c.ref).max()) <= 1e-13 * c.scale, (kind, n, s)
        assert ratios[-1] <= SC.STALL_REGIME or s == 0
        early += any(r1 > 0.1 * r0 and r1 > SC.STALL_REGIME for r0, r1 in zip(ratios, ratios[1:]))
    if n >= 17:
        assert early > 0
