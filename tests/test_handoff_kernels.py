"""The Krylov projection's hand-off kernels against exact references (handoff_cases.py), ONE launch at a time through the
solver's own launchers:
  proxsdp_hip_rotate             Solver::rotate / rotate_launch: k_lz_rotate (one launch or the chunk loop), k_lz_rotate_mfma, k_lzw_rotate
  proxsdp_hip_reconstruct_fused  Solver::launch_reconstruct as ritz_pairs_to_block calls it on the support path:
                                 k_reconstruct_packed<true / false>, k_reconstruct_mfma<true / false>, ldz = npad > n, a block at a
                                 packed offset that is no multiple of 32, residual slots under the XCD permutation
  proxsdp_hip_tail_copy          Solver::launch_tail_copy: k_tail_copy_res

Exact family: whole outputs compared with `==` on bits (small-integer operands: every partial sum in any order is an fp64
number, test_handoff_kernels_host.py holds the bound).  The sentinel every output is prefilled with shows the written set: no
entry of the block left out, nothing behind it, the padding workgroups' residual slots untouched.  Rounded family: one derived
bound per entry; the fused maxima are `==` given the kernel's own block."""
import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import handoff_cases as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert B.device_count() > 0, "no HIP device: the hand-off kernels have no CPU fallback"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(_bits(got).reshape(got.shape) != _bits(exp).reshape(exp.shape))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {got.size} differ, first at {tuple(bad[0])}: "
                           f"{got[tuple(bad[0])]!r} != {exp[tuple(bad[0])]!r}")


# ------------------------------------------------------------------------------------------------ reconstruction
def _reconstruct(cs, mfma, fused=True):
    kw = dict(xold=cs["xold"], mask=cs["mask"], mask_off=cs["mask_off"]) if fused else {}
    out = B.reconstruct_fused(cs["Z"], cs["lam"], cs["n"], mfma=mfma, sentinel=H.SENTINEL, **kw)
    assert out["grid"] == H.grid_of(cs["n"])
    assert np.all(out["guard"] == H.SENTINEL), "a residual slot behind 2 x grid was written"
    if mfma >= 0:
        assert out["kernel"] == ("packed", "mfma")[mfma]
    else:
        assert out["kernel"] == ("mfma" if cs["r"] >= 16 else "packed"), "the auto rule: MFMA from rank 16 on"
    return out


def _check_fused_exact(cs, mfma, what):
    out = _reconstruct(cs, mfma)
    xp = out["xp"]
    assert not np.isnan(xp).any(), (what, "the NaN rows n .. ldz of Z reached the block")
    assert not np.any(xp == H.SENTINEL), (what, "entries never written", np.nonzero(xp == H.SENTINEL)[0][:5])
    _same_bits(xp, cs["xp"], what + " block")
    r = out["respart"]
    for b, t in enumerate(H.slot_tiles(cs["n"])):
        if t is None:
            assert np.all(r[:, b] == H.SENTINEL), (what, "padding workgroup wrote its slot", b, r[:, b])
    _same_bits(r, cs["respart"], what + " off-support maxima per slot")
    return out


@pytest.mark.parametrize("case", H.recon_launch_cases(), ids=lambda c: "n%d-r%d-%s-off%d-mfma%d" % c)
def test_exact_fused_reconstruction(case):
    """The production launch: the block bit for bit, slot b = the maxima of tile xcd_tile(b) over its off-support entries (+0.0
    for an all-on tile), padding slots and the guard zone untouched; the unfused launch with the same ldz gives the same bits."""
    n, r, kind, off, mfma = case
    cs = H.recon_exact_case(n, r, kind, off)
    what = f"n {n} r {r} ldz {kind} mask_off {off} mfma {mfma} ({cs['mask_kind']}, {cs['plant_mode']})"
    out = _check_fused_exact(cs, mfma, what)
    for t in cs["allon"]:
        b = H.slot_tiles(n).index(t)
        assert _bits(out["respart"][:, b]).tolist() == [0, 0], (what, "all-on tile", t)
    if r == 0:
        assert not _bits(out["xp"]).any()                                       # +0.0 everywhere
        off_ = ~cs["on"]
        assert out["respart"][0][[b for b, t in enumerate(H.slot_tiles(n)) if t is not None]].max() == np.abs(cs["xold"][off_]).max(initial=0.0)
    plain = _reconstruct(cs, mfma, fused=False)
    _same_bits(plain["xp"], out["xp"], what + " unfused against fused")
    assert np.all(plain["respart"] == H.SENTINEL), (what, "the unfused launch wrote residual slots")


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("mode", H.PLANT_MODES)
@pytest.mark.parametrize("n", [65, 200])
def test_planted_maxima(n, mode, mfma):
    """Every tile's off-support maximum planted at a chosen place (first / last tile row, diagonal, column n-1, bit 31 / 0 of
    a mask word) between on-support neighbours with |x_old| = 1e30: a bit read one off, in either direction, moves a slot."""
    for seed in range(2):
        cs = H.recon_exact_case(n, 17, "npad", 37, seed=seed, mask_kind="half", plant_mode=mode)
        _check_fused_exact(cs, mfma, f"n {n} {mode} seed {seed} mfma {mfma}")


ORDINARY = [(65, 17), (200, 33), (577, 63)]


def _ordinary(n, r, mfma):
    cs = H.recon_exact_case(n, r, "npad", 4101, seed=1, plant_mode="none")
    return cs, _reconstruct(cs, mfma)


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("n,r", ORDINARY)
def test_ordinary_old_iterate(n, r, mfma):
    """Nothing planted: x_old of the size of x_new, full mantissas, half the entries on the support, so that every slot's maximum
    is an ordinary entry.  The block and max |x_old| bit for bit; max |x_new - x_old| within what a difference formed from the
    unrounded x_new may be off: 2^-53 |x_new| for the product's rounding and one rounding of each of the two results."""
    cs, out = _ordinary(n, r, mfma)
    what = f"n {n} r {r} mfma {mfma}, nothing planted"
    _same_bits(out["xp"], cs["xp"], what + " block")
    res, exp = out["respart"], cs["respart"]
    _same_bits(res[1], exp[1], what + " max |x_old| per slot")
    real = np.array([t is not None for t in H.slot_tiles(n)])
    assert np.all(res[0][~real] == H.SENTINEL) and np.count_nonzero(res[0][real] > 0) >= H.ntiles_of(n) - 1
    bound = H.U53 * (np.abs(cs["xp"]).max() + 2.5 * exp[0][real])
    assert np.all(np.abs(res[0][real] - exp[0][real]) <= bound), (what, np.abs(res[0][real] - exp[0][real]).max())


@pytest.mark.xfail(strict=True, reason="both fused kernels contract x_new - x_old into fma(s, acc, -x_old): the maximum is formed from "
                   "the UNROUNDED x_new, one ulp off the stored one's; switching the contraction off moves the bits_maxcut_* goldens")
@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("n,r", ORDINARY)
def test_maxima_of_an_ordinary_old_iterate(n, r, mfma):
    """The same launches: max |x_new - x_old| with x_new the STORED value -- one rounding of the difference, as NumPy forms it --
    compared with `==` (everything else about them is asserted in test_ordinary_old_iterate).

    KNOWN FAILURE, kept strict.  The compiler fuses `xn = s * acc; ... fabs(xn - xold)` of k_reconstruct_packed<true> and
    k_reconstruct_mfma<true> into one v_fma_f64 per entry (16 of them in each kernel's epilogue, one v_add_f64 left), so the slot
    holds max |fl(s acc - x_old)|, formed from the exact product, not from the stored fl(s acc).  Measured on an MI355X, both
    kernels alike: at n = 65, r = 17 workgroup 1 reports 695.3930100519266 where the stored block gives 695.3930100519267; 1 of
    3, 5 of 10 and 15 of 55 tiles differ at n = 65, 200, 577 -- exactly the slots test_handoff_kernels_host.py predicts for a
    fused multiply-subtract.  With `#pragma clang fp contract(off)` at the head of the two store blocks all six cases pass; but
    the primal residual of every support-path iteration is made of these maxima, and that build leaves
    bits_maxcut_n2000_round3 at row 472 (test_round4_step_kernels_reproduce_round3_bit_for_bit).  So the kernels stay as they
    are and this stays an expected failure: a rewrite of the epilogue that changes the contraction shows here or in the goldens."""
    cs, out = _ordinary(n, r, mfma)
    _same_bits(out["respart"][0], cs["respart"][0], f"n {n} r {r} mfma {mfma}: max |x_new - x_old| per slot")


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("kind", H.MASK_KINDS)
def test_mask_kinds(kind, mfma):
    """all-off (the plain maxima), whole tiles all-on (+0.0), the 1 % density of Max-Cut and 50 %, at a mask offset of 4101"""
    cs = H.recon_exact_case(200, 33, "npad", 4101, seed=3, mask_kind=kind, plant_mode="bit31")
    out = _check_fused_exact(cs, mfma, f"{kind} mfma {mfma}")
    if kind == "alloff":
        assert out["respart"][1].max() == np.abs(cs["xold"]).max()


@pytest.mark.parametrize("mfma", [0, 1])
@pytest.mark.parametrize("n,r", H.RECON_ROUNDED)
def test_rounded_reconstruction_within_the_derived_bound(n, r, mfma):
    cs = H.recon_rounded_case(n, r)
    out = _reconstruct(cs, mfma)
    xp = out["xp"]
    assert not np.any(xp == H.SENTINEL) and not np.isnan(xp).any()
    err = np.abs((xp.astype(np.longdouble) - cs["ref"]).astype(np.float64))
    ratio = float((err / cs["bound"]).max())
    print(f"n {n} r {r} mfma {mfma}: largest error / bound = {ratio:.4f}")
    assert np.all(err <= cs["bound"]), (n, r, mfma, ratio)
    assert ratio > 0
    # the maxima belong to the block the kernel stored: still exact
    _same_bits(out["respart"], H.expected_respart(n, xp, cs["xold"], cs["on"]), f"n {n} r {r} mfma {mfma} maxima of the kernel's own block")
    _same_bits(_reconstruct(cs, mfma, fused=False)["xp"], xp, "unfused against fused")


# ------------------------------------------------------------------------------------------------ rotation
def _rotate(cs, wide=0):
    out = B.rotate(cs["V"], cs["U"], cs["K"], copy_src=cs["copy_src"], copy_dst=cs["copy_dst"], wide=wide,
                   out_cols=cs["out_cols"], sentinel=H.SENTINEL)
    forms, lo, hi = H.rot_form_rule(cs["K"], cs["ncols"], cs["copy_src"] >= 0, wide)
    what = f"n {cs['n']} K {cs['K']} ncols {cs['ncols']} copy {cs['copy_src']} -> {cs['copy_dst']} wide {wide}"
    assert out["form"] in forms, (what, out["form"], forms)
    if out["form"] == "scalar":
        assert lo <= out["launches"] <= hi, (what, out["launches"], lo, hi)
    else:
        assert out["launches"] == (0 if out["form"] == "none" else 1), (what, out["form"], out["launches"])
    return out, what


def _check_rotation_exact(cs, wide=0):
    out, what = _rotate(cs, wide)
    n, nc = cs["n"], cs["ncols"]
    got = out["out"]
    assert not _bits(got[n:, :nc]).any(), (what, "padding rows of the rotated columns are not +0.0")
    _same_bits(got, cs["expected"], what)
    if cs["copy_src"] >= 0:
        _same_bits(got[:n, cs["copy_dst"]], cs["V"][:, cs["copy_src"]], what + " copied column")
    return out


@pytest.mark.parametrize("K", H.ROT_NARROW_K)
def test_exact_rotation_narrow(K):
    """Columns 0 .. ncols-1 = V U in integers, column copy_dst the bits of V[:, copy_src], +0.0 in their padding rows, the
    sentinel in every other column; the form and the number of launches as the launcher's rules say."""
    for row in H.rot_launch_cases(False)[K]:
        _check_rotation_exact(H.rot_exact_case(*row))


@pytest.mark.parametrize("K", H.ROT_WIDE_K)
def test_exact_rotation_wide(K):
    for row in H.rot_launch_cases(True)[K]:
        out = _check_rotation_exact(H.rot_exact_case(*row), wide=1)
        assert out["form"] == "wide"


def test_every_form_is_reached():
    """One shape per form -- single-launch scalar, the chunk loop, MFMA, wide -- reported by the launcher, not assumed"""
    seen = {}
    for n, K, nc, wide in ((65, 31, 17, 0), (65, 64, 16, 0), (65, 127, 78, 0), (65, 255, 100, 0), (65, 300, 65, 1)):
        cs = H.rot_exact_case(n, K, nc, K, nc)
        out = _check_rotation_exact(cs, wide)
        key = out["form"] if out["form"] != "scalar" else ("scalar x1" if out["launches"] == 1 else "scalar chunk loop")
        seen.setdefault(key, []).append((K, nc, out["launches"]))
    print(seen)
    missing = {"scalar x1", "scalar chunk loop", "mfma", "wide"} - set(seen)
    assert not missing, f"forms not reached: {sorted(missing)}; reached {seen}"


@pytest.mark.parametrize("K,ncols", [(3, 3), (33, 17), (64, 64), (127, 78), (205, 80), (255, 100)])
def test_every_form_that_accepts_a_shape_gives_the_same_bits(K, ncols):
    """The same V, U through the narrow launcher (scalar, chunk loop or MFMA) and -- in a workspace of Krylov dimension 256 --
    through the wide kernel: identical bits, and the integer product."""
    big = H.rot_exact_case(65, K, ncols, K, ncols + 3, Kv=257)
    cs = dict(big, V=np.asfortranarray(big["V"][:, :K + 1]))                   # the same columns 0 .. K in a narrow workspace
    narrow = _check_rotation_exact(cs)
    wide = _check_rotation_exact(big, wide=1)
    assert narrow["form"] != "wide" and wide["form"] == "wide"
    _same_bits(wide["out"], narrow["out"], f"K {K} ncols {ncols}: wide against {narrow['form']} x{narrow['launches']}")


@pytest.mark.parametrize("K,wide", [(1, 0), (31, 0), (64, 0), (127, 0), (255, 0), (300, 1)])
def test_copy_only_launch(K, wide):
    """ncols = 0 with a copy writes the copy column and nothing else; without a copy nothing is launched"""
    cs = H.rot_exact_case(65, K, 0, K, 2)
    out = _check_rotation_exact(cs, wide)
    assert out["launches"] == 1 and out["form"] == ("wide" if wide else "scalar")
    assert np.all(out["out"][:, [0, 1, 3, 4]] == H.SENTINEL)
    none = _check_rotation_exact(H.rot_exact_case(65, K, 0, -1, 0), wide)
    assert none["form"] == "none" and np.all(none["out"] == H.SENTINEL)


@pytest.mark.parametrize("n,K,ncols,wide", H.ROT_ROUNDED)
def test_rounded_rotation_within_the_derived_bound(n, K, ncols, wide):
    cs = H.rot_rounded_case(n, K, ncols)
    out = B.rotate(cs["V"], cs["U"], K, copy_src=K, copy_dst=ncols, wide=wide, out_cols=ncols + 2, sentinel=H.SENTINEL)
    got = out["out"]
    err = np.abs((got[:n, :ncols].astype(np.longdouble) - cs["ref"]).astype(np.float64))
    ratio = float((err / cs["bound"]).max())
    print(f"n {n} K {K} ncols {ncols}: {out['form']} x{out['launches']}, largest error / bound = {ratio:.4f}")
    assert np.all(err <= cs["bound"]), (n, K, ncols, out["form"], ratio)
    assert ratio > 0 and not _bits(got[n:, :ncols + 1]).any()
    _same_bits(got[:n, ncols], cs["V"][:, K], "copied column")
    assert np.all(got[:, ncols + 1] == H.SENTINEL)


# ------------------------------------------------------------------------------------------------ tail copy
@pytest.mark.parametrize("wgs", H.TAIL_WGS)
@pytest.mark.parametrize("length", H.TAIL_LENGTHS)
def test_tail_copy(length, wgs):
    """xout[start:] = xin[start:] bit for bit and nothing in front of it; slot 0 of every workgroup +0.0 (x_new = x_old here),
    slot 1 the largest off-support |x| of the workgroup's own grid stride"""
    cs = H.tail_case(length, wgs)
    xout, res = B.tail_copy(cs["x"], cs["start"], cs["mask"], wgs, sentinel=H.SENTINEL)
    exp_x, exp_r = H.tail_expected(cs)
    _same_bits(xout, exp_x, f"tail {length} on {wgs} workgroups: copy")
    assert not _bits(res[0]).any(), "slot 0 is +0.0 in every workgroup"
    _same_bits(res, exp_r, f"tail {length} on {wgs} workgroups: maxima per workgroup")
    off = ~cs["on"][cs["start"]:]
    assert res[1].max() == np.abs(cs["x"][cs["start"]:][off]).max()
