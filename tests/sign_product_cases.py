"""Inputs and references for the kernel-level tests of the sign projection's MFMA products (proxsdp_hip_sym_product: k_sym_gemm,
k_sym_gemm32, k_sym_gemm48 through Solver::sym_gemm) and of its head (proxsdp_hip_sign_unpack: k_unpack_sym, k_sign_scalars);
shared by test_sign_products_host.py (CPU) and test_sign_products.py (GPU).

EXACT family.  Operands are symmetric matrices of dyadic rationals m 2^-b, the coefficients small integers or powers of two,
so that every product P_ik Q_kj, every partial sum of them IN ANY ORDER and every value of the epilogue is a multiple of one
unit 2^-U below 2^53 units: representable in fp64, whatever the waves' split of K, the butterfly's order or the compiler's
contraction.  The reference is an int64 matrix product, scaled; `exact_proof` holds the integer-arithmetic bound.  The kernels
compute the block upper triangle of the product and mirror it, so for non-commuting P, Q the expected matrix is the upper
triangle of P Q and its mirror.

ROUNDED family.  Full-mantissa doubles in production shape; the reference is np.longdouble (asserted to carry >= 63 mantissa
bits, i.e. x87 extended: its own error, K 2^-64, is 2^-11 of the bound), the bound per entry
    (K + 8) 2^-53 (|ka| delta_ij + |kb| |Y_ij| + |kc| (|P| |Q|)_ij),     K = ld,
the any-order dot-product bound plus the epilogue's few roundings (ka, kb, kc themselves, three products, two sums)."""
import functools
import math
import pathlib
import re
from fractions import Fraction

import numpy as np

TILE = 64
SENTINEL = -7.25e300
SQRT2 = 1.41421356237309504880          # kernels.hip.hpp
INV_SQRT2 = 0.70710678118654752440
U53 = 2.0 ** -53

SIDES = {64: (1, 2, 63, 64, 65, 129, 200, 257, 330),
         32: (1, 31, 32, 33, 64, 65, 200),
         48: (47, 48, 49, 96, 144, 145, 192, 240, 100, 250)}
FINAL_SIDES = (5, 64, 65, 200)
UNPACK_SIDES = (1, 2, 64, 65, 200)
ROUNDED_SIDES = (48, 65, 129)


def ld_of(n):
    return TILE * (-(-n // TILE))


def tile48_fits(n):
    """the solver's rule (Solver::sign_tile48_fits, apart from the LDS grant): the 48-tiles must lie inside the padded matrix"""
    return 48 * (-(-n // 48)) <= ld_of(n)


def tiles_per_side(n, tile):
    return {64: ld_of(n) // 64, 32: ld_of(n) // 32, 48: -(-n // 48)}[tile]


def grid_of(n, tile):
    nt = tiles_per_side(n, tile)
    return 8 * (-(-(nt * (nt + 1) // 2) // 8))


def slot_tiles(n, tile):
    """[(I, J) or None] per launched workgroup: the XCD-interleaved order of the kernels (xcd_tile, tile_coords)"""
    nt = tiles_per_side(n, tile)
    ntile = nt * (nt + 1) // 2
    q = (ntile + 7) >> 3
    coords = [(i, j) for j in range(nt) for i in range(j + 1)]          # t = j (j + 1) / 2 + i
    out = []
    for b in range(grid_of(n, tile)):
        t = (b & 7) * q + (b >> 3)
        out.append(coords[t] if t < ntile else None)
    return out


def written_side(n, tile):
    """the kernels write [0, w)^2 of the ld x ld result: everything for 64 / 32, the tiles' own square for 48"""
    return 48 * (-(-n // 48)) if tile == 48 else ld_of(n)


# ------------------------------------------------------------------------------------------------ exact family
def _int_sym(rng, n, M):
    A = rng.integers(-M, M + 1, size=(n, n), dtype=np.int64)
    return np.triu(A) + np.triu(A, 1).T


def _fb(x):
    """fractional bits of a dyadic rational"""
    d = Fraction(x).denominator
    assert d & (d - 1) == 0
    return d.bit_length() - 1


def _lowrank_pair(rng, n):
    """P = u u' + 2^15 w w', Q = v v' + 2^15 z z' with u, v in {-1 .. 1} ({-7 .. 7} for v) paired over DISTANT indices so that
    u'v = 1 by cancellation, and w, z sparse +-1: the true product u (u'v) v' + ... + 2^30 (w'z) w z' has exact zeros, entries
    of size <= 7 and entries beyond 2^30; every k contributes a non-zero term to most entries."""
    u = rng.choice([-1, 1], size=n).astype(np.int64)
    v = np.zeros(n, dtype=np.int64)
    perm = rng.permutation(n)
    nz = max(1, n // 8)                                    # indices where v stays 0: exact zero columns of u v'
    rest = perm[nz:]
    if len(rest) % 2 == 0 and len(rest):
        rest = rest[1:]
    if len(rest):
        v[rest[0]] = u[rest[0]]                            # the one unpaired overlap: u'v = 1
        for a, b in zip(rest[1::2], rest[2::2]):
            t = int(rng.integers(1, 8)) * int(rng.choice([-1, 1]))
            v[a], v[b] = t, -t * u[a] * u[b]               # u_a v_a + u_b v_b = 0
    w = np.zeros(n, dtype=np.int64)
    z = np.zeros(n, dtype=np.int64)
    S = perm[nz:nz + max(1, n // 5)] if n > nz else perm[:1]      # away from the zeros of v: those columns of P Q are exactly 0
    w[S] = rng.choice([-1, 1], size=len(S))
    z[S] = w[S]
    z[S[::3]] *= -1                                        # w'z = |S| - 2 ceil(|S| / 3) != 0 in general
    P = np.outer(u, u) + (1 << 15) * np.outer(w, w)
    Q = np.outer(v, v) + (1 << 15) * np.outer(z, z)
    return P, Q


@functools.lru_cache(maxsize=None)
def exact_cases(n):
    """The exact family at side n: dicts with integer operands Pi, Qi, Yi and their binary scales bp, bq, by (operand = int 2^-b),
    epilogue, ca, cb, cc, dsc (or None)."""
    rng = np.random.default_rng(1000 + n)
    A = _int_sym(rng, n, 7)
    Y = A @ A
    out = []
    # commuting pairs, as in production: polynomials of one integer matrix
    out.append(dict(name="AA", kind="commuting", epilogue="plain", Pi=A, Qi=A, bp=2, bq=2, Yi=None, by=0,
                    ca=0.0, cb=0.0, cc=0.0, dsc=(0.125, 0.0, 0.0)))
    out.append(dict(name="YY", kind="commuting", epilogue="poly", Pi=Y, Qi=Y, bp=4, bq=4, Yi=Y, by=4,
                    ca=3.0, cb=-2.0, cc=1.0, dsc=(2.0, 0.5, 4.0)))
    Qc = 3 * 16 * np.eye(n, dtype=np.int64) - Y            # Q = 3 I - (A/4)^2 at scale 2^-4: commutes with X = A / 4
    out.append(dict(name="XQ", kind="commuting", epilogue="plain", Pi=A, Qi=Qc, bp=2, bq=4, Yi=None, by=0,
                    ca=0.0, cb=0.0, cc=0.0, dsc=None))
    # generic non-commuting symmetric P != Q, 20-bit entries
    M = (1 << 20) - 1
    Pg, Qg, Yg = _int_sym(rng, n, M), _int_sym(rng, n, M), _int_sym(rng, n, M)
    out.append(dict(name="generic", kind="generic", epilogue="poly", Pi=Pg, Qi=Qg, bp=20, bq=7, Yi=Yg, by=9,
                    ca=-2.0, cb=0.5, cc=2.0, dsc=(1.0, 4.0, 0.5)))
    # low rank, sign-alternating: cancellation to exact zeros beside entries 2^30 apart
    for _ in range(64):                                    # (redrawn until every aligned group of 4, 8, 16 k contributes: no chance zeros)
        Pl, Ql = _lowrank_pair(rng, n)
        if all(np.any(Pl[:, k0:k0 + st] @ Ql[k0:k0 + st, :]) for st in (4, 8, 16) for k0 in range(0, n, st)):
            break
    out.append(dict(name="lowrank", kind="lowrank", epilogue="plain", Pi=Pl, Qi=Ql, bp=0, bq=3, Yi=None, by=0,
                    ca=0.0, cb=0.0, cc=0.0, dsc=None))
    return out


def operands(cs):
    """fp64 operands of a case (exact: integers of at most 37 bits times a power of two)"""
    P = cs["Pi"].astype(np.float64) * 2.0 ** -cs["bp"]
    Q = cs["Qi"].astype(np.float64) * 2.0 ** -cs["bq"]
    Y = cs["Yi"].astype(np.float64) * 2.0 ** -cs["by"] if cs["Yi"] is not None else None
    return P, Q, Y


def coefficients(cs):
    """(ka, kb, kc) as the kernels form them: ca m0, cb m1, cc m2 for poly, (0, 0, m0) for plain and final"""
    m = cs["dsc"] if cs["dsc"] is not None else (1.0, 1.0, 1.0)
    if cs["epilogue"] == "poly":
        return cs["ca"] * m[0], cs["cb"] * m[1], cs["cc"] * m[2]
    return 0.0, 0.0, m[0]


def exact_proof(cs, final=False):
    """Integer arithmetic only.  With unit = 2^-U the finest scale any term lives on, returns (units of the largest possible
    |value| of an entry at ANY stage -- sum_k |P_ik| |Q_kj| scaled by |kc|, plus the other terms --, U).  Below 2^53 units every
    intermediate and every result is an fp64 number."""
    ka, kb, kc = (Fraction(c) for c in coefficients(cs))
    Pa, Qa = np.abs(cs["Pi"]), np.abs(cs["Qi"])
    assert int(Pa.max()) * int(Qa.max()) * cs["Pi"].shape[0] < 2 ** 62          # the int64 products below cannot wrap
    dot = int((Pa @ Qa).max())                                                  # any-order bound of the dot products
    # (coefficient, largest integer magnitude, binary scale of that integer): value <= coefficient * magnitude * 2^-scale
    terms = [(abs(kc), dot, cs["bp"] + cs["bq"]), (Fraction(1), dot, cs["bp"] + cs["bq"])]
    if cs["epilogue"] == "poly":
        terms += [(abs(ka), 1, 0), (abs(kb), int(np.abs(cs["Yi"]).max()), cs["by"])]
    if final:                                                                   # (P + m0 P Q): the epilogue operand is P
        terms += [(Fraction(1), int(Pa.max()), cs["bp"])]
    U = max(e + _fb(c) for c, _, e in terms)
    total = sum(c * m * Fraction(2) ** (U - e) for c, m, e in terms)
    assert total.denominator == 1
    return int(total), U


def expected_full(cs):
    """exact value of the epilogue on the full n x n product P Q (not yet triangle + mirror), as fp64"""
    n = cs["Pi"].shape[0]
    ka, kb, kc = coefficients(cs)
    PQ = (cs["Pi"] @ cs["Qi"]).astype(np.float64) * 2.0 ** -(cs["bp"] + cs["bq"])
    E = kc * PQ
    if cs["epilogue"] == "poly":
        E = E + kb * (cs["Yi"].astype(np.float64) * 2.0 ** -cs["by"]) + ka * np.eye(n)
    return E


def expected_T(cs, tile, sentinel=SENTINEL):
    """the whole ld x ld output: upper triangle of the epilogue of P Q, its mirror below; the padding inside the written square
    zero (poly: ka on the diagonal); `sentinel` where the 48-tiles do not reach"""
    n = cs["Pi"].shape[0]
    ld, w = ld_of(n), written_side(n, tile)
    E = expected_full(cs)
    T = np.full((ld, ld), sentinel)
    T[:w, :w] = 0.0
    T[:n, :n] = np.triu(E) + np.triu(E, 1).T
    if cs["epilogue"] == "poly":
        ka = coefficients(cs)[0]
        idx = np.arange(n, w)
        T[idx, idx] = ka
    return T


def fro_units(cs, tile):
    """(sum over the written square of T^2 in units 2^-2U as a Python int, U): the Frobenius partials are sums of non-negative
    multiples of that unit, so every partial sum in any order is at most this total -- exact in fp64 iff it is below 2^53"""
    n = cs["Pi"].shape[0]
    _, U = exact_proof(cs)
    w = written_side(n, tile)
    Tw = expected_T(cs, tile)[:w, :w] * 2.0 ** U
    Ti = Tw.astype(np.int64)
    assert np.array_equal(Ti.astype(np.float64), Tw)
    return sum(int(v) * int(v) for v in Ti.ravel()), U


def expected_part(cs, tile):
    """per launched workgroup: the Frobenius^2 partial of its tile (upper-triangle entries counted twice, as the kernels do),
    0.0 for a padding workgroup"""
    n = cs["Pi"].shape[0]
    T = expected_T(cs, tile, sentinel=0.0)
    out = []
    for ij in slot_tiles(n, tile):
        if ij is None:
            out.append(0.0)
            continue
        I, J = ij
        B = T[I * tile:(I + 1) * tile, J * tile:(J + 1) * tile]
        out.append(float(np.sum(np.triu(B) ** 2) * 2 - np.sum(np.diag(B) ** 2)) if I == J else float(2 * np.sum(B ** 2)))
    return np.array(out)


# ------------------------------------------------------------------------------------------------ final product
def packed_index(n):
    """(gi, gj) of every packed entry, column-major upper triangle"""
    gj = np.repeat(np.arange(n), np.arange(1, n + 1))
    gi = np.concatenate([np.arange(j + 1) for j in range(n)])
    return gi, gj


@functools.lru_cache(maxsize=None)
def final_case(n, variant):
    """SG_FINAL at side n.  variant: "plain" (no residuals, m0 = 1/2 from dsc), or a fused-residual layout:
    "diag" / "lastcol": the largest |x+ - xold| of the off-support entries planted on the diagonal / in the last column, with
    larger differences on ON-support neighbours of it (a mask or xold read one entry off finds those);
    "empty": a whole tile (n > 64) or the whole block on the support: no off-support entry there;
    "clamp": the last column off the support with |xold| >= 1000 x the largest difference -- the lanes of the last tile with
    gj >= n read exactly those entries (indices clamped to n - 1) and must ignore them."""
    rng = np.random.default_rng(7000 + 10 * n + ["plain", "diag", "lastcol", "empty", "clamp"].index(variant))
    M = (1 << 12) - 1
    P, Q = _int_sym(rng, n, M), _int_sym(rng, n, M)
    cs = dict(name=f"final-{variant}", kind="final", epilogue="final" if variant == "plain" else "final_res", Pi=P, Qi=Q,
              bp=3, bq=5, Yi=None, by=0, ca=0.0, cb=0.0, cc=0.0, dsc=(0.5, 0.0, 0.0) if variant == "plain" else None)
    gi, gj = packed_index(n)
    N = len(gi)
    E = expected_full(cs)                                   # m0 P Q
    Pf = P.astype(np.float64) * 2.0 ** -cs["bp"]
    v = Pf[gi, gj] + E[gi, gj]                              # exact
    cs["xp"] = np.where(gi == gj, 0.5, 0.5 * SQRT2) * v     # ONE rounding per entry: fl(c v)
    cs["trace_q"] = float(np.trace(Q)) * 2.0 ** -cs["bq"]
    if variant == "plain":
        return cs
    mask_off = {5: 37, 64: 1000003, 65: 31, 200: 4097}[n]
    bits = rng.integers(0, 2, size=mask_off + N + 64).astype(bool)      # on and off bits side by side in every word
    delta = rng.uniform(-1.0, 1.0, size=N)
    xold = cs["xp"] + delta
    on = bits[mask_off:mask_off + N]                        # a view: edits below land in bits
    tile_of = (gi // TILE, gj // TILE)
    if variant in ("diag", "lastcol"):
        cand = np.nonzero((gi == gj) if variant == "diag" else ((gj == n - 1) & (gi < gj) if n > 1 else gi == gj))[0]
        k = int(cand[len(cand) // 2])
        on[k] = False
        xold[k] = cs["xp"][k] + 64.0
        for nb in (k - 1, k + 1):                           # ON-support neighbours with a larger difference
            if 0 <= nb < N:
                on[nb] = True
                xold[nb] = cs["xp"][nb] - 1024.0
        cs["planted"] = k
    elif variant == "empty":
        if n > TILE:
            sel = (tile_of[0] == (n - 1) // TILE - (1 if n >= 192 else 0)) & (tile_of[1] == (n - 1) // TILE)
        else:
            sel = np.ones(N, dtype=bool)
        on[sel] = True
        cs["empty_sel"] = sel
    elif variant == "clamp":
        on[gj == n - 1] = False                             # (the differences stay |delta| <= 1; x+ itself supplies the magnitude)
    nw = len(bits) // 32                                    # bit b of word k = bits[32 k + b]
    mask = (bits[:32 * nw].reshape(nw, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    assert len(mask) * 32 >= mask_off + N
    assert all(bool((mask[(mask_off + k) >> 5] >> ((mask_off + k) & 31)) & 1) == bool(on[k]) for k in (0, N // 2, N - 1))
    cs.update(xold=xold, mask=mask, mask_off=mask_off, on=on.copy())
    # per launched workgroup (64-tiles): max |x+ - xold| and max |xold| over its OFF-support entries
    diff, mag = np.abs(cs["xp"] - xold), np.abs(xold)
    r = np.zeros((2, grid_of(n, 64)))
    for b, ij in enumerate(slot_tiles(n, 64)):
        if ij is None:
            continue
        sel = (tile_of[0] == ij[0]) & (tile_of[1] == ij[1]) & ~on
        if sel.any():
            r[0, b], r[1, b] = diff[sel].max(), mag[sel].max()
    cs["respart"] = r
    return cs


def expected_trace_part(cs):
    n = cs["Qi"].shape[0]
    d = np.diag(cs["Qi"]).astype(np.float64) * 2.0 ** -cs["bq"]
    return np.array([0.0 if (ij is None or ij[0] != ij[1]) else float(d[ij[0] * TILE:(ij[0] + 1) * TILE].sum())
                     for ij in slot_tiles(n, 64)])


# ------------------------------------------------------------------------------------------------ rounded family
def sign_table():
    """(rows, last_cubic) of csrc/sign_table.inc"""
    txt = (pathlib.Path(__file__).resolve().parent.parent / "proxsdp.jl_amd" / "csrc" / "sign_table.inc").read_text()
    rows = [tuple(float(x) for x in m) for m in re.findall(r"^\s*\{([-\d.e]+), ([-\d.e]+), ([-\d.e]+)\}", txt, re.M)]
    assert len(rows) == int(re.search(r"SIGN_STEPS = (\d+)", txt).group(1))
    return rows, "SIGN_LAST_CUBIC = true" in txt


def rounded_matrix(n):
    """a scaled random symmetric A (full mantissas) and its packed svec form (off-diagonals x sqrt 2)"""
    rng = np.random.default_rng(4200 + n)
    A = rng.standard_normal((n, n)) * 37.0
    A = np.triu(A) + np.triu(A, 1).T
    gi, gj = packed_index(n)
    return A, np.where(gi == gj, 1.0, SQRT2) * A[gi, gj]


def rounded_cases(A, sc):
    """Products of a projection's first steps on A, with the device scalars sc of its head (proxsdp_hip_sign_unpack, or
    host_scalars): Y0 = A A / f^2; row 0 of the table on Y0 with dsc = {1, 1/g, 1/g^2}; row 8 on Y = Y0 / g, no dsc; the last,
    cubic row (1.5, 0, -0.5) on X = A / s."""
    rows, cubic = sign_table()
    assert cubic
    Y0 = (A @ A) * sc[0]
    Y0 = np.triu(Y0) + np.triu(Y0, 1).T
    Y8 = Y0 * sc[9]
    X = A * sc[1]
    z = (0.0, 0.0, 0.0)
    return [dict(name="Y0", epilogue="plain", P=A, Q=A, Y=None, c=z, dsc=(sc[0], 0.0, 0.0)),
            dict(name="row0", epilogue="poly", P=Y0, Q=Y0, Y=Y0, c=rows[0], dsc=tuple(sc[8:11])),
            dict(name="row8", epilogue="poly", P=Y8, Q=Y8, Y=Y8, c=rows[8], dsc=None),
            dict(name="cubic", epilogue="poly", P=X, Q=X, Y=X, c=(1.5, 0.0, -0.5), dsc=None)]


def host_scalars(A):
    """what k_sign_scalars stages 0 / 1 define, evaluated in NumPy: the slots of sc the rounded cases use"""
    sc = np.zeros(16)
    f2 = float(np.sum(A * A))
    sc[0], sc[6] = 1.0 / f2, math.sqrt(f2)
    g = math.sqrt(float(np.sum(((A @ A) * sc[0]) ** 2)))
    sc[1], sc[4], sc[8], sc[9], sc[10] = 1.0 / (sc[6] * math.sqrt(g)), sc[6] * math.sqrt(g), 1.0, 1.0 / g, 1.0 / (g * g)
    return sc


def rounded_reference(cs):
    """(reference of the n x n result in np.longdouble, bound per entry in fp64).  The coefficients are the fp64 inputs'
    products taken in extended precision: the kernel's rounding of ka, kb, kc is part of the bound's + 8."""
    L = np.longdouble
    assert np.finfo(L).nmant >= 63, "np.longdouble is not extended precision here"
    n = cs["P"].shape[0]
    m = cs["dsc"] if cs["dsc"] is not None else (1.0, 1.0, 1.0)
    if cs["epilogue"] == "poly":
        ka, kb, kc = L(cs["c"][0]) * L(m[0]), L(cs["c"][1]) * L(m[1]), L(cs["c"][2]) * L(m[2])
    else:
        ka, kb, kc = L(0), L(0), L(m[0])
    P, Q = cs["P"].astype(L), cs["Q"].astype(L)
    ref = kc * (P @ Q)
    mag = abs(float(kc)) * (np.abs(cs["P"]) @ np.abs(cs["Q"]))
    if cs["epilogue"] == "poly":
        ref = ref + kb * cs["Y"].astype(L) + ka * np.eye(n, dtype=L)
        mag = mag + abs(float(kb)) * np.abs(cs["Y"]) + abs(float(ka)) * np.eye(n)
    return ref, (ld_of(n) + 8) * U53 * mag


def rounded_numpy(cs):
    """the same product in plain fp64 NumPy"""
    n = cs["P"].shape[0]
    m = cs["dsc"] if cs["dsc"] is not None else (1.0, 1.0, 1.0)
    if cs["epilogue"] == "poly":
        return (cs["c"][2] * m[2]) * (cs["P"] @ cs["Q"]) + (cs["c"][1] * m[1]) * cs["Y"] + (cs["c"][0] * m[0]) * np.eye(n)
    return m[0] * (cs["P"] @ cs["Q"])


# ------------------------------------------------------------------------------------------------ unpack
def unpack_reference(xp, n):
    """(A n x n with off-diagonals fl(x INV_SQRT2), f^2 by math.fsum of the exactly squared entries, relative any-order bound)"""
    gi, gj = packed_index(n)
    vals = np.where(gi == gj, xp, xp * INV_SQRT2)
    A = np.zeros((n, n))
    A[gi, gj] = vals
    A[gj, gi] = vals
    sq = [Fraction(float(v)) ** 2 * (1 if i == j else 2) for v, i, j in zip(vals, gi, gj)]
    f2 = sum(sq)
    # one rounding per term (none where the compiler fuses it into the sum), at most one per addition of the len(sq) terms in
    # any order -- lanes, waves, workgroup partials, k_sign_scalars' own sum
    return A, f2, (len(sq) + 2) * U53
