"""CPU checks of the fixtures and references of the hand-off kernel tests (handoff_cases.py): the exact families cannot leave
53 bits, the slot map is the brute-force loop's, every generated support layout has the properties its GPU test relies on, the
rounded bounds already hold for a plain fp64 NumPy evaluation, the shape lists reach every mechanism, the binding mirrors the
header's structs and the entries refuse invalid arguments before they touch a device."""
import ctypes
import re

import numpy as np
import pytest

from proxsdp_jl_amd import binding as B

import handoff_cases as H

STRUCTS = {"proxsdp_reconstruct_fused": B.ReconstructFusedIO, "proxsdp_rotation": B.RotationIO, "proxsdp_tail_copy": B.TailCopyIO}
ENTRIES = {"proxsdp_hip_reconstruct_fused", "proxsdp_hip_rotate", "proxsdp_hip_tail_copy"}


def _named(header, name):
    """the header declares `typedef struct { .. } name;`: give the struct its name for test_host_abi's field parser"""
    m = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} " + name + ";", header, re.S)
    return "typedef struct " + name + " {" + m.group(1) + "} " + name + ";"


def test_binding_exposes_the_entries_and_mirrors_the_structs():
    assert B.lib().proxsdp_hip_abi_version() == 10
    assert ENTRIES <= set(B.header_symbols())
    assert all(hasattr(B.lib(), e) for e in ENTRIES)
    assert callable(B.reconstruct_fused) and callable(B.rotate) and callable(B.tail_copy)
    import test_host_abi as T
    header = B.HEADER_PATH.read_text()
    for name, cls in STRUCTS.items():
        assert [f for f, _ in cls._fields_] == T._c_struct_fields(_named(header, name), name), name
    # every member is 4 or 8 bytes wide and the 4-byte ones come in pairs: no padding, the size is the sum
    assert ctypes.sizeof(B.ReconstructFusedIO) == 8 + 4 * 4 + 8 * 4 + 8 * 2 + 8 + 8 + 8 * 2 + 4 * 2 == 112
    assert ctypes.sizeof(B.RotationIO) == 8 + 4 * 8 + 8 * 2 + 8 + 8 + 4 * 4 == 88
    assert ctypes.sizeof(B.TailCopyIO) == 8 + 8 * 2 + 8 * 3 + 4 * 2 + 8 + 8 * 2 == 80
    forms = {int(v): k for k, v in re.findall(r"#define PROXSDP_ROTATE_(\w+)\s+(\d+)", header)}
    assert forms == {1: "SCALAR", 2: "MFMA", 3: "WIDE"} and {k: v.upper() for k, v in B.ROTATE_FORMS.items() if k} == forms
    assert B.SYM_SENTINEL == H.SENTINEL


def test_invalid_arguments_are_refused_before_the_device_is_touched():
    """code -1 with or without a GPU: ldz < n, a short mask, ncols > K, wide without the wide workspace"""
    cs = H.recon_exact_case(5, 3, "n", 37)
    with pytest.raises(B.ProxSDPHipError, match="ldz < n") as e:
        B.reconstruct_fused(cs["Z"][:4], cs["lam"], 5, xold=cs["xold"], mask=cs["mask"], mask_off=37)
    assert e.value.code == -1
    short = cs["mask"][:(37 + 15) // 32]                       # 32 bits for bit numbers up to 51
    with pytest.raises(B.ProxSDPHipError, match="mask does not cover") as e:
        B.reconstruct_fused(cs["Z"], cs["lam"], 5, xold=cs["xold"], mask=short, mask_off=37)
    assert e.value.code == -1
    with pytest.raises(B.ProxSDPHipError, match="mask does not cover") as e:
        B.reconstruct_fused(cs["Z"], cs["lam"], 5, xold=cs["xold"], mask=cs["mask"], mask_off=-1)
    assert e.value.code == -1
    V, U = np.ones((5, 4)), np.ones((3, 4))
    with pytest.raises(B.ProxSDPHipError, match="ncols must be 0 .. K") as e:
        B.rotate(V, U, 3)
    assert e.value.code == -1
    with pytest.raises(B.ProxSDPHipError, match="wide = 1 needs the wide workspace") as e:
        B.rotate(np.ones((5, 65)), np.ones((64, 16)), 64, wide=1)
    assert e.value.code == -1
    with pytest.raises(B.ProxSDPHipError, match="Krylov dimension out of range") as e:
        B.rotate(np.ones((5, 257)), np.ones((256, 1)), 256, wide=0)
    assert e.value.code == -1
    with pytest.raises(B.ProxSDPHipError, match="too few columns") as e:
        B.rotate(np.ones((5, 4)), np.ones((4, 1)), 4, copy_src=4, copy_dst=1)
    assert e.value.code == -1
    with pytest.raises(B.ProxSDPHipError, match="outside out") as e:
        B.rotate(np.ones((5, 5)), np.ones((4, 1)), 4, copy_src=4, copy_dst=3, out_cols=3)
    assert e.value.code == -1
    tc = H.tail_case(257, 2)
    with pytest.raises(B.ProxSDPHipError, match="mask does not cover") as e:
        B.tail_copy(tc["x"], tc["start"], tc["mask"][:tc["N"] // 32], 2)
    assert e.value.code == -1
    with pytest.raises(B.ProxSDPHipError, match="start must be") as e:
        B.tail_copy(tc["x"], tc["N"], tc["mask"], 2)
    assert e.value.code == -1


def test_without_a_device_the_entries_fail_loudly():
    if B.device_count() > 0:
        pytest.skip("a GPU is present")
    cs = H.recon_exact_case(5, 3, "npad", 37)
    with pytest.raises(B.ProxSDPHipError) as e:
        B.reconstruct_fused(cs["Z"], cs["lam"], 5, xold=cs["xold"], mask=cs["mask"], mask_off=37)
    assert e.value.code == -2
    with pytest.raises(B.ProxSDPHipError) as e:
        B.rotate(np.ones((5, 4)), np.ones((3, 2)), 3)
    assert e.value.code == -2
    tc = H.tail_case(1, 1)
    with pytest.raises(B.ProxSDPHipError) as e:
        B.tail_copy(tc["x"], tc["start"], tc["mask"], 1)
    assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ layout
@pytest.mark.parametrize("n", H.RECON_SIDES + (129, 449, 1000))
def test_slot_map_is_the_brute_force_loop(n):
    slots = H.slot_tiles(n)
    assert slots == H.slot_tiles_brute(n) and len(slots) == H.grid_of(n)
    real = [t for t in slots if t is not None]
    assert sorted(real) == list(range(H.ntiles_of(n)))                          # every tile exactly once
    coords = H.tile_coords_brute(n)
    gi, gj, tile = H.packed_index(n)
    assert len(coords) == H.ntiles_of(n) and np.array_equal(gj * (gj + 1) // 2 + gi, np.arange(len(gi)))
    for t, (I, J) in enumerate(coords):
        assert I <= J and t == J * (J + 1) // 2 + I
    k = np.arange(0, len(gi), max(1, len(gi) // 211))
    assert all(coords[tile[q]] == (gi[q] // 64, gj[q] // 64) for q in k)


def test_reconstruction_shapes_reach_every_mechanism():
    assert [(H.ntiles_of(n), H.grid_of(n)) for n in (1, 5, 63, 64)] == [(1, 8)] * 4
    assert [(H.ntiles_of(n), H.grid_of(n)) for n in (65, 130, 200, 577)] == [(3, 8), (6, 8), (10, 16), (55, 56)]
    for n in (200, 577):                                                        # padding workgroups and a real permutation
        slots = H.slot_tiles(n)
        assert None in slots and [t for t in slots if t is not None] != sorted(t for t in slots if t is not None)
    cases = H.recon_launch_cases()
    assert len(cases) == len(set(cases))
    for mfma in (0, 1):
        mine = [c for c in cases if c[4] == mfma]
        assert {c[0] for c in mine} == set(H.RECON_SIDES), mfma
        assert {c[1] for c in mine} == set(H.RECON_RANKS), mfma
        assert {c[2] for c in mine} == set(H.LDZ_KINDS), mfma
        assert {c[3] for c in mine} == set(H.MASK_OFFS), mfma
        assert {c[0] for c in mine if c[3] != 0} == set(H.RECON_SIDES), mfma
    auto = [c for c in cases if c[4] == -1]
    assert {15, 16} <= {c[1] for c in auto}                                     # the auto rule's cross-over
    assert all(off % 32 != 0 for off in H.MASK_OFFS if off) and 4101 > 64 * 65 // 2
    kinds = {H.recon_exact_case(*c[:4])["mask_kind"] for c in cases}
    modes = {H.recon_exact_case(*c[:4])["plant_mode"] for c in cases}
    assert kinds == set(H.MASK_KINDS) and modes == set(H.PLANT_MODES)


@pytest.mark.parametrize("case", H.recon_launch_cases(), ids=lambda c: "n%d-r%d-%s-off%d-mfma%d" % c)
def test_exact_reconstruction_cases_hold_what_the_gpu_test_relies_on(case):
    n, r, kind, off, _ = case
    cs = H.recon_exact_case(n, r, kind, off)
    _check_headroom_and_layout(cs)
    assert cs["Z"].shape == (H.ldz_of(n, kind), r) and np.isnan(cs["Z"][n:]).all() and not np.isnan(cs["Z"][:n]).any()
    if r >= 3:
        assert (cs["li"] == 0).any() and (cs["li"] < 0).any() and (cs["li"] > 0).any()
    # the packed reference: integer on the diagonal, ONE rounding of SQRT2 * integer off it
    gi, gj, _ = H.packed_index(n)
    M = (cs["Zi"].astype(object) * cs["li"].astype(object)) @ cs["Zi"].astype(object).T if r else np.zeros((n, n), dtype=object)
    for k in {0, len(gi) // 2, len(gi) - 1}:
        v = int(M[gi[k], gj[k]])
        assert cs["xp"][k] == (float(v) if gi[k] == gj[k] else H.SQRT2 * float(v)) and abs(v) < 2 ** 53
    if r == 0:
        assert not cs["xp"].any() and not np.signbit(cs["xp"]).any()


def _check_headroom_and_layout(cs):
    n = cs["n"]
    if "Zi" in cs:
        head = H.recon_headroom(cs["Zi"], cs["li"])
        assert head <= 600 * 7 * 225 < 2 ** 53 and np.abs(cs["Zi"]).max(initial=0) <= 15 and np.abs(cs["li"]).max(initial=0) <= 7
    gi, gj, tile = H.packed_index(n)
    on, xold, off = cs["on"], cs["xold"], cs["mask_off"]
    N = len(gi)
    assert len(cs["mask"]) * 32 >= off + N
    assert all(H.mask_bit(cs["mask"], off + k) == bool(on[k]) for k in range(0, N, max(1, N // 199)))
    if off:
        words = cs["mask"][off // 32:(off + N + 31) // 32]
        if cs["mask_kind"] == "half" and N >= 64:
            assert np.any((words != 0) & (words != 0xFFFFFFFF))                 # on and off bits inside one word
    diff = np.abs(cs["xp"] - xold) if "xp" in cs else None
    for t in range(H.ntiles_of(n)):
        mem = tile == t
        if t in cs["allon"]:
            assert on[mem].all()                                                # designated all-on tiles really are all-on
            continue
        assert not on[mem].all()                                                # every other tile has an off-support entry
        k = cs["planted"][t]
        assert mem[k] and not on[k] and abs(xold[k]) == H.PLANT
        others = mem & ~on
        others[k] = False
        assert np.abs(xold[others]).max(initial=0.0) < H.PLANT
        if diff is not None:
            assert diff[k] >= H.PLANT > diff[others].max(initial=0.0)           # the planted entry alone carries both maxima
    assert np.all(np.abs(xold[on]) == H.HUGE)
    for t, k in cs["planted"].items():
        if cs["mask_kind"] != "alloff":
            near = [q for q in (k - 1, k + 1) if 0 <= q < N and q not in cs["planted"].values() and tile[q] not in cs["allon"]]
            assert all(on[q] for q in near)                                     # one bit off in either direction: a HUGE entry
    if "respart" in cs:
        r = cs["respart"]
        assert r.shape == (2, H.grid_of(n))
        for b, t in enumerate(H.slot_tiles(n)):
            if t is None:
                assert np.all(r[:, b] == H.SENTINEL)
            elif t in cs["allon"]:
                assert np.all(r[:, b] == 0.0) and not np.signbit(r[:, b]).any()
            else:
                k = cs["planted"][t]
                assert r[0, b] == abs(cs["xp"][k] - xold[k]) and r[1, b] == H.PLANT


@pytest.mark.parametrize("mode", H.PLANT_MODES)
@pytest.mark.parametrize("n", [65, 200])
def test_planted_positions_are_where_the_mode_says(n, mode):
    gi, gj, tile = H.packed_index(n)
    hits = 0
    for seed in range(3):
        cs = H.recon_exact_case(n, 17, "npad", 37, seed=seed, mask_kind="half", plant_mode=mode)
        _check_headroom_and_layout(cs)
        for t, k in cs["planted"].items():
            I, J = H.tile_coords_brute(n)[t]
            at = lambda q: dict(first_row=gi[q] == 64 * I, last_row=gi[q] == min(64 * I + 63, n - 1), diag=gi[q] == gj[q],
                                lastcol=gj[q] == n - 1, bit31=(37 + q) % 32 == 31, bit0=(37 + q) % 32 == 0)[mode]
            ok = at(k)
            possible = any(at(q) for q in np.nonzero(tile == t)[0])             # (a tile of one entry has no bit 31)
            assert ok or not possible, (t, k)
            hits += bool(ok)
    assert hits >= 3


@pytest.mark.parametrize("n,r", [(65, 17), (200, 33), (577, 63)])
def test_ordinary_old_iterate_case(n, r):
    """nothing planted: the slots' maxima are ordinary entries, and a contracted sqrt(2) m - x_old (ONE rounding of the exact
    value, not of the stored x_new's difference) would move some of them"""
    from fractions import Fraction
    cs = H.recon_exact_case(n, r, "npad", 4101, seed=1, plant_mode="none")
    assert not cs["planted"] and not cs["allon"] and np.abs(cs["xold"]).max() < 1e7
    assert H.recon_headroom(cs["Zi"], cs["li"]) < 2 ** 53
    gi, gj, tile = H.packed_index(n)
    res = cs["respart"]
    differ = 0
    for b, t in enumerate(H.slot_tiles(n)):
        if t is None:
            continue
        mem = np.nonzero((tile == t) & ~cs["on"])[0]
        if not len(mem):
            continue
        d = np.abs(cs["xp"][mem] - cs["xold"][mem])
        k = mem[int(np.argmax(d))]
        assert res[0, b] == d.max() and res[1, b] == np.abs(cs["xold"][mem]).max()
        if gi[k] != gj[k]:
            m = int(((cs["Zi"][gi[k]] * cs["li"]) @ cs["Zi"][gj[k]]))
            fused = float(abs(Fraction(H.SQRT2) * m - Fraction(float(cs["xold"][k]))))      # one rounding of the exact value
            differ += fused != res[0, b]
    print(f"n={n}: {differ} slot maxima would change under a fused multiply-subtract")
    if n >= 200:
        assert differ > 0


@pytest.mark.parametrize("n,r", H.RECON_ROUNDED)
def test_rounded_reconstruction_bound_holds_for_plain_numpy(n, r):
    assert np.finfo(np.longdouble).nmant >= 63
    cs = H.recon_rounded_case(n, r)
    _check_headroom_and_layout(cs)
    err = np.abs((H.recon_numpy(cs).astype(np.longdouble) - cs["ref"]).astype(np.float64))
    ratio = float((err / cs["bound"]).max())
    print(f"n={n} r={r}: NumPy fp64 error / bound = {ratio:.3f}")
    assert np.all(err <= cs["bound"]) and 0 < ratio < 1
    assert np.all(np.frexp(cs["Z"][:n])[0] * 2.0 ** 53 % 2 ** 20 != 0)          # full mantissas


# ------------------------------------------------------------------------------------------------ rotation
def test_rotation_shapes_reach_every_mechanism():
    narrow, wide = H.rot_launch_cases(False), H.rot_launch_cases(True)
    assert tuple(narrow) == H.ROT_NARROW_K and tuple(wide) == H.ROT_WIDE_K
    for K, rows in list(narrow.items()) + list(wide.items()):
        table = H.ROT_WIDE_NCOLS if K > 255 else H.ROT_NCOLS
        assert {r[2] for r in rows} >= {min(c, K) for c in table}, K
        for n, K_, nc, cs_, cd in rows:
            assert K_ == K and n in H.ROT_SIDES and 0 <= nc <= K and cs_ in (-1, K) and (cs_ < 0 or cd in (nc, nc + 3) or nc == 0)
    flat = [r for rows in narrow.values() for r in rows] + [r for rows in wide.values() for r in rows]
    assert {r[0] for r in flat} == set(H.ROT_SIDES)
    assert {(r[3] >= 0, r[4] - r[2]) for r in flat if r[2] > 0} >= {(False, -r[2]) for r in flat if r[3] < 0 and r[2] > 0} | {(True, 0), (True, 3)}
    assert any(r[2] == 0 and r[3] >= 0 for r in flat)                           # the copy-only launch
    p = H.ROT_PRODUCTION
    assert (p["n"], p["K"], p["ncols"], p["copy_src"], p["copy_dst"]) in narrow[127]
    # the switch rules, over every LDS grant: K = 204 is the last MFMA fit, K >= 205 with >= 16 columns is the chunk loop
    assert H.rot_mfma_lds(204) <= H.ROT_MFMA_LDS_MAX < H.rot_mfma_lds(205)
    assert H.rot_form_rule(31, 31, False, False)[0] == {"scalar"} and H.rot_form_rule(64, 15, False, False)[0] == {"scalar"}
    assert H.rot_form_rule(32, 16, False, False)[0] == {"mfma", "scalar"}
    forms, lo, hi = H.rot_form_rule(255, 100, True, False)
    assert forms == {"scalar"} and lo == 7 and hi > lo
    assert H.rot_form_rule(205, 100, False, False)[1] >= 2
    assert H.rot_form_rule(300, 0, True, True) == ({"wide"}, 1, 1) and H.rot_form_rule(64, 0, False, False) == ({"none"}, 0, 0)
    assert H.rot_scalar_launches(127, 78, True, 160 * 1024) == 1                # the production restart is ONE launch
    assert any(K % 2 for K in H.ROT_NARROW_K) and any(K % 4 for K in H.ROT_NARROW_K if K >= 32)


@pytest.mark.parametrize("K", H.ROT_NARROW_K + H.ROT_WIDE_K)
def test_exact_rotation_cases_stay_inside_53_bits(K):
    for n, K_, nc, cs_, cd in H.rot_launch_cases(K > 255)[K]:
        cs = H.rot_exact_case(n, K, nc, cs_, cd)
        assert H.rot_headroom(cs["Vi"], cs["Ui"], K) <= 511 * 49 < 2 ** 53
        assert np.abs(cs["Vi"]).max() <= 7 and np.abs(cs["Ui"]).max(initial=0) <= 7
        E = cs["expected"]
        assert E.shape == (H.npad_of(n), cs["out_cols"])
        assert np.array_equal(E[:n, :nc], (cs["Vi"][:, :K].astype(object) @ cs["Ui"].astype(object)).astype(np.float64))
        assert not E[n:, :nc].any() and np.all(E[:, -2:] == H.SENTINEL)
        written = set(range(nc)) | ({cd} if cs_ >= 0 else set())
        for c in range(cs["out_cols"]):
            assert (c in written) != bool(np.all(E[:, c] == H.SENTINEL))
        if nc:
            # the last basis column contributes to every entry: a dropped odd-K tail cannot hide
            assert np.all(cs["Vi"][:, K - 1] != 0) and np.all(cs["Ui"][K - 1] != 0)


@pytest.mark.parametrize("n,K,ncols,wide", H.ROT_ROUNDED)
def test_rounded_rotation_bound_holds_for_plain_numpy(n, K, ncols, wide):
    assert np.finfo(np.longdouble).nmant >= 63
    cs = H.rot_rounded_case(n, K, ncols)
    err = np.abs(((cs["V"][:, :K] @ cs["U"]).astype(np.longdouble) - cs["ref"]).astype(np.float64))
    ratio = float((err / cs["bound"]).max())
    print(f"n={n} K={K} ncols={ncols}: NumPy fp64 error / bound = {ratio:.3f}")
    assert np.all(err <= cs["bound"]) and 0 < ratio < 1
    assert np.abs(cs["U"].T @ cs["U"] - np.eye(ncols)).max() < 1e-12


# ------------------------------------------------------------------------------------------------ tail copy
@pytest.mark.parametrize("wgs", H.TAIL_WGS)
@pytest.mark.parametrize("length", H.TAIL_LENGTHS)
def test_tail_cases(length, wgs):
    assert H.TAIL_START % 32 and H.TAIL_START % 256
    cs = H.tail_case(length, wgs)
    xout, res = H.tail_expected(cs)
    s, N = cs["start"], cs["N"]
    assert N - s == length and np.all(xout[:s] == H.SENTINEL) and np.array_equal(xout[s:], cs["x"][s:])
    assert all(H.mask_bit(cs["mask"], k) == bool(cs["on"][k]) for k in range(0, N, max(1, N // 199)))
    assert not res[0].any() and res.shape == (2, wgs)
    off = ~cs["on"][s:]
    assert res[1].max() == np.abs(cs["x"][s:][off]).max() == 1000.0
    # a plain loop over the grid stride of every workgroup
    if length <= 257 or wgs == 256:
        for w in range(wgs):
            m = 0.0
            for base in range(s + 256 * w, N, 256 * wgs):
                for i in range(base, min(base + 256, N)):
                    if not cs["on"][i]:
                        m = max(m, abs(cs["x"][i]))
            assert res[1, w] == m, w
    if length > 2:
        assert cs["on"][s + 1] and abs(cs["x"][s + 1]) == H.HUGE                # one on-support bit read as off swamps the slot
    assert np.abs(cs["x"][:s][~cs["on"][:s]]).max() > 1000.0                    # an entry in front of `start` would show
