"""Inputs and references for the kernel-level tests of the Krylov projection's hand-off: the basis rotation (proxsdp_hip_rotate:
k_lz_rotate, k_lz_rotate_mfma, k_lzw_rotate through Solver::rotate / rotate_launch), the rank-r reconstruction with the fused
off-support maxima (proxsdp_hip_reconstruct_fused: k_reconstruct_packed<FUSE_RES> / k_reconstruct_mfma<FUSE_RES> through
Solver::launch_reconstruct) and the tail copy (proxsdp_hip_tail_copy: k_tail_copy_res); shared by
test_handoff_kernels_host.py (CPU) and test_handoff_kernels.py (GPU).

EXACT family.  Small-integer operands: Z in [-15, 15], lam in [-7, 7] (sum_k |lam z z| <= 600 * 7 * 225 < 2^53), V and U in
[-7, 7].  Every product and every partial sum IN ANY ORDER -- scalar chains, MFMA steps, chunked or not, contracted or not -- is
an integer below 2^53, i.e. an fp64 number: the reference is an int64 product.  The packed block is that integer on the diagonal
and fl(SQRT2 * integer) off it: ONE rounding, the same in NumPy.  `recon_headroom` / `rot_headroom` hold the bound.

ROUNDED family.  Standard-normal / orthonormal operands; the reference is np.longdouble (x87 extended, >= 63 mantissa bits:
asserted on the host), whose own error terms * 2^-64 * sum is added to the bound:
    reconstruction  |got - ref| <= (r + 8) 2^-53 s_ij sum_k |lam_k Z_ik Z_jk|     (one rounding for lam z, at most one per
                    accumulation step, one for the SQRT2 product, the constant's own error; + 8 as sign_product_cases.py)
    rotation        |got - ref| <= (K + 8) 2^-53 sum_j |V_ij| |U_jc|.

The fused maxima are max |x_new - x_old| and max |x_old| over a tile's off-support entries, with x_new the value the kernel
stored: one rounding per difference, compared with `==` in both families."""
import functools

import numpy as np

TILE = 64
TPB = 256
SENTINEL = -7.25e300
SQRT2 = 1.41421356237309504880          # kernels.hip.hpp
U53 = 2.0 ** -53
U64 = 2.0 ** -64
HUGE = 1e30                             # |x_old| of the on-support entries: one of them read as off-support swamps its slot
PLANT = 2.0 ** 40                       # |x_old| of a tile's planted off-support maximum: above every other off-support value

RECON_SIDES = (1, 5, 63, 64, 65, 130, 200, 577)
RECON_RANKS = (0, 1, 3, 15, 16, 17, 31, 32, 33, 63, 64, 130)
LDZ_KINDS = ("n", "npad", "npad+64")
MASK_OFFS = (0, 37, 4101)
MASK_KINDS = ("alloff", "allon_tiles", "sparse", "half")
PLANT_MODES = ("first_row", "last_row", "diag", "lastcol", "bit31", "bit0")

ROT_SIDES = (1, 64, 65, 200)
ROT_NARROW_K = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 204, 205, 255)
ROT_NCOLS = (0, 1, 3, 15, 16, 17, 33, 64, 80, 100)
ROT_WIDE_K = (256, 257, 300, 511)
ROT_WIDE_NCOLS = (1, 63, 64, 65, 130)
ROT_PRODUCTION = dict(n=200, K=127, ncols=78, copy_src=127, copy_dst=78)     # the rank-63 restart: krylovdim 127, keep 78

TAIL_LENGTHS = (1, 255, 256, 257, 70001)
TAIL_WGS = (1, 2, 256)
TAIL_START = 4133                       # 129 * 32 + 5: no multiple of 32 or 256


# ------------------------------------------------------------------------------------------------ layout
def npad_of(n):
    return TILE * (-(-n // TILE))


def ntiles_of(n):
    nt = -(-n // TILE)
    return nt * (nt + 1) // 2


def grid_of(n):
    """workgroups of a reconstruction launch: the tiles of the block triangle, padded to the 8 XCDs"""
    return 8 * (-(-ntiles_of(n) // 8))


def xcd_tile(b, ntile):
    """kernels.hip.hpp xcd_tile: the tile workgroup b works on (>= ntile: a padding workgroup)"""
    q = (ntile + 7) >> 3
    return (b & 7) * q + (b >> 3)


def slot_tiles(n):
    """[tile or None] per launched workgroup (= per residual slot)"""
    nt = ntiles_of(n)
    return [t if t < nt else None for t in (xcd_tile(b, nt) for b in range(grid_of(n)))]


def slot_tiles_brute(n):
    """The same map from its description, as a plain loop: XCD x (the workgroups b = x, x + 8, x + 16, ...) walks the contiguous
    tile range [x q, (x + 1) q) in order, q = ceil(ntile / 8); whatever lies beyond the last tile is padding."""
    nt = ntiles_of(n)
    q = -(-nt // 8)
    out = [None] * grid_of(n)
    for x in range(8):
        for k in range(q):
            t = x * q + k
            b = x + 8 * k
            if b < len(out) and t < nt:
                out[b] = t
    return out


def tile_coords_brute(n):
    """[(I, J)] per linear tile id: column-major over the upper block triangle (kernels.hip.hpp tile_coords)"""
    nt = -(-n // TILE)
    return [(i, j) for j in range(nt) for i in range(j + 1)]


@functools.lru_cache(maxsize=None)
def packed_index(n):
    """(gi, gj, tile) of every packed entry: idx = gj (gj + 1) / 2 + gi, tile = J (J + 1) / 2 + I"""
    gj = np.repeat(np.arange(n), np.arange(1, n + 1))
    gi = np.arange(n * (n + 1) // 2) - gj * (gj + 1) // 2
    I, J = gi // TILE, gj // TILE
    return gi, gj, J * (J + 1) // 2 + I


def mask_words(on, mask_off, rng):
    """uint32 words of a support mask whose bit mask_off + k is on[k]; the bits in front of and behind the block are random"""
    nbits = 32 * (-(-(mask_off + len(on)) // 32) + 2)
    bits = rng.integers(0, 2, size=nbits).astype(bool)
    bits[mask_off:mask_off + len(on)] = on
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").ravel().astype(np.uint32)


def mask_bit(mask, g):
    return bool((int(mask[g >> 5]) >> (g & 31)) & 1)


# ------------------------------------------------------------------------------------------------ reconstruction
def recon_launch_cases():
    """(n, r, ldz kind, mask_off, mfma) of the exact family: every side, rank, ldz kind and mask offset with BOTH kernels forced,
    every side with a mask offset != 0 (test_handoff_kernels_host.py checks exactly that), then the auto rule at its cross-over."""
    out = []
    for mfma in (0, 1):
        for i, r in enumerate(RECON_RANKS):
            n = RECON_SIDES[(i + 3 * mfma) % len(RECON_SIDES)]
            out.append((n, r, LDZ_KINDS[(i + mfma) % 3], MASK_OFFS[(i + 1 + mfma) % 3], mfma))
    # the sides the walk above meets with mask offset 0 only
    out += [(130, 33, "npad", 37, 0), (63, 17, "npad", 4101, 1), (577, 63, "npad", 37, 1)]
    out += [(65, 15, "npad", 37, -1), (65, 16, "npad", 37, -1), (130, 0, "n", 4101, -1), (200, 130, "npad+64", 0, -1)]
    return out


def ldz_of(n, kind):
    return {"n": n, "npad": npad_of(n), "npad+64": npad_of(n) + 64}[kind]


def padded(Z, ldz):
    """Z with its rows n .. ldz-1 filled with NaN: padding the kernels must never read"""
    n, r = Z.shape
    out = np.full((ldz, r), np.nan, order="F")
    out[:n] = Z
    return out


def recon_integers(n, r, seed):
    """Zi (n x r) in [-15, 15], li (r) in [-7, 7] with a zero and negatives among them, M = Z diag(lam) Z' (int64)"""
    rng = np.random.default_rng([7001, n, r, seed])
    Zi = rng.integers(-15, 16, size=(n, r), dtype=np.int64)
    li = rng.integers(-7, 8, size=r, dtype=np.int64)
    if r >= 2:
        li[-1] = -(abs(int(li[-1])) or 2)
        li[0] = abs(int(li[0])) or 3
    if r >= 3:
        li[rng.integers(1, r - 1)] = 0
    return Zi, li, (Zi * li) @ Zi.T


def recon_headroom(Zi, li):
    """the largest sum_k |lam_k Z_ik Z_jk|: every partial sum of the products, in any order, stays below it"""
    return int(((np.abs(Zi) * np.abs(li)) @ np.abs(Zi).T).max(initial=0))


def packed_from_matrix(M):
    """xp of an exactly known matrix: the entry on the diagonal, fl(SQRT2 * entry) off it"""
    n = M.shape[0]
    gi, gj, _ = packed_index(n)
    v = M[gi, gj].astype(np.float64)
    return np.where(gi == gj, v, SQRT2 * v)


def support_layout(n, xp, mask_off, mask_kind, plant_mode, seed):
    """on (bool per packed entry), xold, mask words and the planted entry of every tile for one fused launch.
    on-support entries carry |xold| = HUGE (and so a huge |xp - xold|): one of them read as off-support swamps its slot.  Every
    tile that is not all-on gets ONE planted off-support entry with xold = -+PLANT, sign against xp: it alone is the tile's
    max |xp - xold| and max |xold|, so that bit read as on changes both slots.  Its neighbours in bit order are on-support."""
    rng = np.random.default_rng([7002, n, mask_off, seed])
    gi, gj, tile = packed_index(n)
    N, nt = len(gi), ntiles_of(n)
    if plant_mode == "none":
        # nothing planted: x_old of the size of x_new with full mantissas, so that every slot's maximum is an ordinary entry and
        # the ONE rounding of x_new - x_old (x_new as stored) is what the comparison sees
        on = rng.random(N) < 0.5
        xold = xp * (1.0 + 0.25 * rng.standard_normal(N)) + 3.0 * rng.standard_normal(N)
        return dict(on=on, xold=xold, mask=mask_words(on, mask_off, rng), mask_off=mask_off, planted={}, allon=[],
                    mask_kind="half", plant_mode="none")
    if mask_kind == "alloff":
        on = np.zeros(N, dtype=bool)
    elif mask_kind == "sparse":
        on = rng.random(N) < 0.01
    else:
        on = rng.random(N) < 0.5
    allon = sorted({0, nt - 1}) if mask_kind == "allon_tiles" else []
    for t in allon:
        on[tile == t] = True
    xold = rng.standard_normal(N) * 50.0
    pred = dict(first_row=gi % TILE == 0, last_row=gi == np.minimum((gi // TILE) * TILE + TILE - 1, n - 1), diag=gi == gj,
                lastcol=gj == n - 1, bit31=(mask_off + np.arange(N)) % 32 == 31, bit0=(mask_off + np.arange(N)) % 32 == 0)[plant_mode]
    planted = {}
    for t in range(nt):
        if t in allon:
            continue
        members = np.nonzero(tile == t)[0]
        cand = members[pred[members]]
        k = int(rng.choice(cand if len(cand) else members))
        planted[t] = k
        on[k] = False
        for q in (k - 1, k + 1):
            if 0 <= q < N and q not in planted.values() and mask_kind != "alloff" and tile[q] not in allon:
                on[q] = True
    for t, k in planted.items():
        on[k] = False
    xold[on] = np.where(rng.random(int(on.sum())) < 0.5, -HUGE, HUGE)
    for k in planted.values():
        xold[k] = -PLANT if xp[k] >= 0 else PLANT
    return dict(on=on, xold=xold, mask=mask_words(on, mask_off, rng), mask_off=mask_off, planted=planted, allon=allon,
                mask_kind=mask_kind, plant_mode=plant_mode)


def expected_respart(n, xp, xold, on):
    """(2, grid): slot b = the maxima of tile xcd_tile(b) over its off-support entries (+0.0 without any), SENTINEL in the slots
    of the padding workgroups: they are zeroed once at set-up and never written again"""
    _, _, tile = packed_index(n)
    nt = ntiles_of(n)
    m = np.zeros((2, nt))
    off = ~on
    np.maximum.at(m[0], tile[off], np.abs(xp[off] - xold[off]))
    np.maximum.at(m[1], tile[off], np.abs(xold[off]))
    out = np.full((2, grid_of(n)), SENTINEL)
    for b, t in enumerate(slot_tiles(n)):
        if t is not None:
            out[:, b] = m[:, t]
    return out


def recon_exact_case(n, r, ldz_kind, mask_off, seed=0, mask_kind=None, plant_mode=None):
    Zi, li, M = recon_integers(n, r, seed)
    xp = packed_from_matrix(M)
    mask_kind = mask_kind or MASK_KINDS[(n + r + seed) % len(MASK_KINDS)]
    plant_mode = plant_mode or PLANT_MODES[(n + r + seed) % len(PLANT_MODES)]
    cs = support_layout(n, xp, mask_off, mask_kind, plant_mode, seed)
    cs.update(n=n, r=r, Zi=Zi, li=li, Z=padded(Zi.astype(np.float64), ldz_of(n, ldz_kind)), lam=li.astype(np.float64), xp=xp,
              mask_kind=mask_kind, plant_mode=plant_mode, respart=expected_respart(n, xp, cs["xold"], cs["on"]))
    return cs


RECON_ROUNDED = ((65, 17), (130, 63), (64, 130), (200, 33))


def recon_rounded_case(n, r):
    """orthonormal columns where they exist (r <= n), standard normal otherwise; lam standard normal"""
    rng = np.random.default_rng([7003, n, r])
    Z = rng.standard_normal((n, r))
    if r <= n:
        Z = np.linalg.qr(Z)[0]
    lam = rng.standard_normal(r) * 3.0
    gi, gj, _ = packed_index(n)
    Zl, ll = Z.astype(np.longdouble), lam.astype(np.longdouble)
    s = np.where(gi == gj, np.longdouble(1), np.sqrt(np.longdouble(2)))
    ref = s * ((Zl * ll) @ Zl.T)[gi, gj]
    mag = (s * ((np.abs(Zl) * np.abs(ll)) @ np.abs(Zl).T)[gi, gj]).astype(np.float64)
    bound = (r + 8) * U53 * mag + (r + 2) * U64 * mag
    xp64 = ref.astype(np.float64)
    cs = support_layout(n, xp64, 37, "half", "diag", 5)
    cs.update(n=n, r=r, Z=padded(Z, npad_of(n)), lam=lam, ref=ref, bound=bound, mag=mag)
    return cs


def recon_numpy(cs):
    """the packed block from a plain fp64 NumPy evaluation (the bound must already hold for it)"""
    n = cs["n"]
    Z = cs["Z"][:n]
    gi, gj, _ = packed_index(n)
    return np.where(gi == gj, 1.0, SQRT2) * ((Z * cs["lam"]) @ Z.T)[gi, gj]


# ------------------------------------------------------------------------------------------------ rotation
def rot_ncols(K, table=ROT_NCOLS):
    """the column counts of the table, clipped to K, each once"""
    return sorted({min(c, K) for c in table})


def rot_copy_variants(K, ncols):
    """(copy_src, copy_dst): none, the residual column K to ncols (a restart) and to ncols + 3"""
    return [(-1, 0), (K, ncols), (K, ncols + 3)]


def rot_launch_cases(wide):
    """(n, K, ncols, copy_src, copy_dst) of the exact family, grouped by K: every ncols of the table with every K, sides and copy
    variants walked so that each appears with every K group; the production-shaped case rides with the narrow K = 127."""
    out = {}
    for a, K in enumerate(ROT_WIDE_K if wide else ROT_NARROW_K):
        rows = []
        for b, nc in enumerate(rot_ncols(K, ROT_WIDE_NCOLS if wide else ROT_NCOLS)):
            n = ROT_SIDES[(a + b) % len(ROT_SIDES)]
            cs_, cd = rot_copy_variants(K, nc)[(a + 2 * b) % 3]
            if nc == 0:
                cs_, cd = K, (0, 3)[a % 2]                      # the copy-only launch
            rows.append((n, K, nc, cs_, cd))
        if K == 127 and not wide:
            p = ROT_PRODUCTION
            rows.append((p["n"], p["K"], p["ncols"], p["copy_src"], p["copy_dst"]))
        out[K] = rows
    return out


def rot_integers(n, K, ncols, Kv, seed=0):
    rng = np.random.default_rng([7004, n, K, ncols, seed])
    Vi = rng.integers(-7, 8, size=(n, Kv), dtype=np.int64)
    Ui = rng.integers(-7, 8, size=(K, ncols), dtype=np.int64)
    Vi[:, K - 1] = np.where(Vi[:, K - 1] == 0, 3, Vi[:, K - 1])        # the last basis column always contributes:
    if ncols:
        Ui[K - 1] = np.where(Ui[K - 1] == 0, -2, Ui[K - 1])            # a dropped odd-K tail shows in every entry
    return Vi, Ui


def rot_headroom(Vi, Ui, K):
    return int((np.abs(Vi[:, :K]) @ np.abs(Ui)).max(initial=0))


def rot_expected(V, U, K, copy_src, copy_dst, out_cols):
    """npad x out_cols: the product in columns 0 .. ncols-1 and the copy in column copy_dst, +0.0 in their padding rows, the
    sentinel everywhere else"""
    n, ncols = V.shape[0], U.shape[1]
    out = np.full((npad_of(n), out_cols), SENTINEL, order="F")
    out[:, :ncols] = 0.0
    out[:n, :ncols] = V[:, :K] @ U
    if copy_src >= 0:
        out[:, copy_dst] = 0.0
        out[:n, copy_dst] = V[:, copy_src]
    return out


def rot_out_cols(ncols, copy_src, copy_dst):
    """two columns beyond the last one written: they must keep the sentinel"""
    return max(ncols, copy_dst + 1 if copy_src >= 0 else 0) + 2


def rot_exact_case(n, K, ncols, copy_src, copy_dst, Kv=None, seed=0):
    Kv = Kv or K + 1
    Vi, Ui = rot_integers(n, K, ncols, Kv, seed)
    V, U = np.asfortranarray(Vi, dtype=np.float64), np.asfortranarray(Ui, dtype=np.float64)
    oc = rot_out_cols(ncols, copy_src, copy_dst)
    return dict(n=n, K=K, ncols=ncols, copy_src=copy_src, copy_dst=copy_dst, Vi=Vi, Ui=Ui, V=V, U=U, out_cols=oc,
                expected=rot_expected(V, U, K, copy_src, copy_dst, oc))


# smallest and largest dynamic LDS the solver may have been granted (Solver::setup_device)
ROT_LDS_MIN, ROT_LDS_MAX = 60 * 1024, 160 * 1024
ROT_MFMA_LDS_MAX = 156 * 1024


def rot_mfma_lds(K):
    Kp = (K + 3) & ~3
    return (Kp * (TILE + 16) + 16 * (Kp + 2)) * 8


def rot_scalar_launches(K, ncols, copy, cap):
    """launches of rotate_launch's chunk loop under an LDS grant of `cap` bytes"""
    vbytes = K * (TILE + 1) * 8
    maxcols = max(1, (cap - vbytes) // (8 * K))
    if ncols == 0:
        return 1 if copy else 0
    return -(-ncols // maxcols)


def rot_form_rule(K, ncols, copy, wide):
    """(forms the launcher may report, least and most launches) for a shape, over every LDS grant the runtime may have given"""
    if ncols == 0 and not copy:
        return {"none"}, 0, 0
    if wide:
        return {"wide"}, 1, 1
    lo, hi = rot_scalar_launches(K, ncols, copy, ROT_LDS_MAX), rot_scalar_launches(K, ncols, copy, ROT_LDS_MIN)
    if K < 32 or ncols < 16:
        return {"scalar"}, lo, hi
    if rot_mfma_lds(K) > ROT_MFMA_LDS_MAX:
        return {"scalar"}, lo, hi
    return {"mfma", "scalar"}, 1, hi


ROT_ROUNDED = ((200, 127, 78, 0), (65, 33, 17, 0), (200, 255, 100, 0), (64, 300, 65, 1), (1, 64, 64, 0))


def rot_rounded_case(n, K, ncols):
    rng = np.random.default_rng([7005, n, K, ncols])
    V = rng.standard_normal((n, K + 1))
    if n >= K + 1:
        V = np.linalg.qr(V)[0]
    U = np.linalg.qr(rng.standard_normal((K, K)))[0][:, :ncols]
    Vl, Ul = V[:, :K].astype(np.longdouble), U.astype(np.longdouble)
    ref = Vl @ Ul
    mag = (np.abs(Vl) @ np.abs(Ul)).astype(np.float64)
    return dict(n=n, K=K, ncols=ncols, V=np.asfortranarray(V), U=np.asfortranarray(U), ref=ref, mag=mag,
                bound=(K + 8) * U53 * mag + (K + 2) * U64 * mag)


# ------------------------------------------------------------------------------------------------ tail copy
def tail_case(length, wgs, seed=0):
    """x of N = TAIL_START + length entries, a half-on mask with the largest |x| of the tail ON the support and the largest
    off-support value planted in the tail's last entry"""
    rng = np.random.default_rng([7006, length, wgs, seed])
    N = TAIL_START + length
    x = rng.standard_normal(N) * 10.0
    on = rng.random(N) < 0.5
    on[N - 1] = False
    x[N - 1] = -1000.0
    if length > 2:
        on[TAIL_START + 1] = True
        x[TAIL_START + 1] = HUGE
    x[:TAIL_START][~on[:TAIL_START]] *= 1e6                    # off-support values in FRONT of the tail: never looked at
    return dict(N=N, start=TAIL_START, wgs=wgs, x=x, on=on, mask=mask_words(on, 0, rng))


def tail_expected(cs):
    """xout and (2, wgs) residual slots: workgroup w owns the entries start + 256 w + t + 256 wgs k"""
    N, start, wgs = cs["N"], cs["start"], cs["wgs"]
    xout = np.full(N, SENTINEL)
    xout[start:] = cs["x"][start:]
    i = np.arange(start, N)
    owner = ((i - start) // TPB) % wgs
    res = np.zeros((2, wgs))
    off = ~cs["on"][start:]
    np.maximum.at(res[1], owner[off], np.abs(cs["x"][start:][off]))
    return xout, res
