"""The sign projection's MFMA product kernels against exact products (sign_product_cases.py), ONE launch at a time through
proxsdp_hip_sym_product -- Solver::sym_gemm itself: k_sym_gemm<SG_PLAIN / SG_POLY / SG_FINAL, with and without fused residuals>,
k_sym_gemm32<SG_PLAIN / SG_POLY>, k_sym_gemm48<SG_PLAIN / SG_POLY, 4> -- and its head through proxsdp_hip_sign_unpack
(k_unpack_sym, k_sign_scalars stages 0 / 1).

Exact family: the whole ld x ld output, the packed x+, the trace partials and the fused maxima are compared with `==` on bits
(every intermediate is an fp64 number in any order: test_sign_products_host.py holds the proof); the Frobenius partials too
where their sum stays inside 53 bits, else under the any-order bound.  The sentinel the outputs are prefilled with shows the
written set.  Rounded family: one derived bound per entry, (K + 8) 2^-53 (|ka| delta_ij + |kb| |Y_ij| + |kc| (|P| |Q|)_ij)."""
import math

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import sign_product_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert B.device_count() > 0, "no HIP device: the product path has no CPU fallback"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(_bits(got).reshape(got.shape) != _bits(exp).reshape(exp.shape))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {got.size} differ, first at {tuple(bad[0])}: "
                           f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


def _launch(cs, tile, **kw):
    P, Q, Y = S.operands(cs)
    return B.sym_product(P, Q, tile=tile, epilogue=cs["epilogue"], Y=Y, ca=cs["ca"], cb=cs["cb"], cc=cs["cc"], dsc=cs["dsc"],
                         sentinel=S.SENTINEL, **kw)


@pytest.mark.parametrize("tile,n", [(t, n) for t in (64, 32, 48) for n in S.SIDES[t]])
def test_exact_products_and_written_set(tile, n):
    """Commuting, generic and low-rank pairs: T bit for bit over ld x ld -- upper triangle of the product, its mirror, the
    padding rule (zero; poly: ka on the diagonal), the sentinel where the 48-tiles do not reach --, every part slot written."""
    if tile == 48 and not S.tile48_fits(n):
        # the solver's own rule: 48 ceil(n / 48) > ld
        with pytest.raises(B.ProxSDPHipError, match="48 x 48 tiles do not fit") as e:
            _launch(S.exact_cases(n)[0], 48)
        assert e.value.code == -1
        return
    ld = S.ld_of(n)
    for cs in S.exact_cases(n):
        what = f"tile {tile} n {n} {cs['name']}"
        out = _launch(cs, tile)
        assert out["ld"] == ld and out["grid"] == S.grid_of(n, tile), what
        _same_bits(out["T"], S.expected_T(cs, tile), what + " T")
        part, exp = out["part"], S.expected_part(cs, tile)
        slots = S.slot_tiles(n, tile)
        assert not np.any(part == S.SENTINEL), (what, "part slot left unset", np.nonzero(part == S.SENTINEL)[0])
        for b, ij in enumerate(slots):
            if ij is None:
                assert part[b] == 0.0 and not np.signbit(part[b]), (what, "padding workgroup", b, part[b])
        fro, U = S.fro_units(cs, tile)
        if fro < 2 ** 53:
            _same_bits(part, exp, what + " part")
            if cs["epilogue"] == "plain":
                assert math.fsum(part) == float(np.sum(out["T"][:n, :n] ** 2)) == fro * 4.0 ** -U, what
        else:
            # beyond 53 bits: sums of non-negative terms in any order, one rounding per term and per addition
            terms = tile * tile
            assert np.all(np.abs(part - exp) <= (2 * terms + 8) * S.U53 * exp), (what, np.abs(part / np.maximum(exp, 1e-300) - 1).max())


@pytest.mark.parametrize("tile", [64, 32, 48])
def test_partials_are_optional(tile):
    """part = NULL, as most products of the iteration run: the same T"""
    n = 96
    for cs in S.exact_cases(n)[:2]:
        out = _launch(cs, tile, want_part=False)
        assert out["part"] is None
        _same_bits(out["T"], S.expected_T(cs, tile), f"tile {tile} {cs['name']} without partials")


@pytest.mark.parametrize("tile", [32, 48])
@pytest.mark.parametrize("epilogue", ["final", "final_res"])
def test_final_epilogues_are_refused_on_small_tiles(tile, epilogue):
    cs = S.final_case(64, "plain" if epilogue == "final" else "diag")
    P, Q, _ = S.operands(cs)
    with pytest.raises(B.ProxSDPHipError, match="64 x 64 tiles only") as e:
        B.sym_product(P, Q, tile=tile, epilogue=epilogue, xold=cs.get("xold"), mask=cs.get("mask"), mask_off=cs.get("mask_off", 0))
    assert e.value.code == -1


@pytest.mark.parametrize("n", S.FINAL_SIDES)
def test_final_product_exact(n):
    """SG_FINAL: packed x+ = fl(c (P + m0 P Q)) with the kernel's own c = 0.5 / 0.5 SQRT2, trace partials of Q per slot"""
    cs = S.final_case(n, "plain")
    P, Q, _ = S.operands(cs)
    out = B.sym_product(P, Q, tile=64, epilogue="final", dsc=cs["dsc"], sentinel=S.SENTINEL)
    assert out["grid"] == S.grid_of(n, 64)
    _same_bits(out["xp"], cs["xp"], f"final n {n} x+")
    _same_bits(out["part"], S.expected_trace_part(cs), f"final n {n} trace partials")
    assert math.fsum(out["part"]) == cs["trace_q"]


@pytest.mark.parametrize("variant", ["diag", "lastcol", "empty", "clamp"])
@pytest.mark.parametrize("n", S.FINAL_SIDES)
def test_final_product_with_fused_residuals_exact(n, variant):
    """SG_FINAL with the fused off-support maxima: per workgroup max |x+ - xold| and max |xold| over the entries whose support
    bit is clear, 0 for tiles without any and for padding workgroups; x+ and the trace as without them."""
    cs = S.final_case(n, variant)
    P, Q, _ = S.operands(cs)
    out = B.sym_product(P, Q, tile=64, epilogue="final_res", xold=cs["xold"], mask=cs["mask"], mask_off=cs["mask_off"],
                        sentinel=S.SENTINEL)
    what = f"final_res n {n} {variant}"
    _same_bits(out["xp"], cs["xp"], what + " x+")
    _same_bits(out["part"], S.expected_trace_part(cs), what + " trace partials")
    assert not np.any(out["respart"] == S.SENTINEL), (what, "respart slot left unset")
    _same_bits(out["respart"], cs["respart"], what + " residual maxima")
    assert out["respart"][0].max() == np.abs(cs["xp"] - cs["xold"])[~cs["on"]].max(initial=0.0)


@pytest.fixture(scope="module")
def heads():
    """proxsdp_hip_sign_unpack of the rounded matrices, once per side"""
    out = {}
    for n in sorted(set(S.UNPACK_SIDES) | set(S.ROUNDED_SIDES)):
        A, xp = S.rounded_matrix(n)
        out[n] = (A, xp) + B.sign_unpack(xp, n, sentinel=S.SENTINEL)
    return out


@pytest.mark.parametrize("n", S.UNPACK_SIDES)
def test_unpack_and_scalars(heads, n):
    A, xp, Ad, sc = heads[n]
    ld = S.ld_of(n)
    R, f2, rel = S.unpack_reference(xp, n)
    assert Ad.shape == (ld, ld)
    _same_bits(Ad[:n, :n], R, f"unpack n {n}: diagonal as given, off-diagonals fl(x INV_SQRT2), both halves")
    assert np.array_equal(Ad[:n, :n], Ad[:n, :n].T)
    pad = np.ones((ld, ld), dtype=bool)
    pad[:n, :n] = False
    assert np.all(Ad[pad] == S.SENTINEL), "k_unpack_sym wrote into the padding"
    # sc[6] = fl(sqrt(tot)), sc[0] = fl(1 / tot) with tot the any-order sum of the squares
    f2 = float(f2)
    print(f"unpack n {n}: f^2 relative error {abs(sc[6] ** 2 / f2 - 1):.3e}, bound {rel:.3e}")
    assert abs(sc[6] - math.sqrt(f2)) <= (rel / 2 + 2 * S.U53) * math.sqrt(f2)
    assert abs(sc[0] - 1.0 / f2) <= (rel + 2 * S.U53) / f2
    # the scale of the iteration: s = f sqrt(g) >= ||A||_2
    g = 1.0 / sc[9]
    assert sc[8] == 1.0 and abs(sc[10] * g * g - 1) <= 8 * S.U53 and abs(sc[4] * sc[1] - 1) <= 8 * S.U53
    assert abs(sc[4] / (sc[6] * math.sqrt(g)) - 1) <= 8 * S.U53
    lam = np.abs(np.linalg.eigvalsh(R)).max()
    print(f"unpack n {n}: s / ||A||_2 = {sc[4] / lam:.17g}")
    assert sc[4] >= lam
    assert not sc[[2, 3, 5, 7]].any() and not sc[11:].any()


@pytest.mark.parametrize("tile", [64, 32, 48])
@pytest.mark.parametrize("n", S.ROUNDED_SIDES)
def test_rounded_products_within_the_derived_bound(heads, tile, n):
    A, xp, Ad, sc = heads[n]
    worst = 0.0
    for cs in S.rounded_cases(Ad[:n, :n].copy(), sc):
        out = B.sym_product(cs["P"], cs["Q"], tile=tile, epilogue=cs["epilogue"], Y=cs["Y"], ca=cs["c"][0], cb=cs["c"][1],
                            cc=cs["c"][2], dsc=cs["dsc"], sentinel=S.SENTINEL, want_part=False)
        T = out["T"][:n, :n]
        assert np.array_equal(T, T.T)
        ref, bound = S.rounded_reference(cs)
        err = np.abs((T.astype(np.longdouble) - ref).astype(np.float64))
        ratio = float((err / bound).max())
        print(f"tile {tile} n {n} {cs['name']}: largest error / bound = {ratio:.4f}")
        assert np.all(err <= bound), (tile, n, cs["name"], ratio)
        worst = max(worst, ratio)
    assert worst > 0
