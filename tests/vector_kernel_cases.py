"""Inputs and NumPy references for the kernel-level tests of the linesearch batch (proxsdp_hip_trial_batch) and of the
cone tail (proxsdp_hip_cone_tail); shared by test_vector_kernels_host.py (CPU) and test_vector_kernels.py (GPU).

References.  Element-wise results are the fp64 NumPy expressions of pdhg.jl:547-575 / residuals.jl:2-71, one rounding per
product and per sum (NumPy does not fuse).  A column dot is  acc = 0.0; acc += val[k] * y[row[k]]  over the column's entries
in CSC STORAGE order (col_dots below runs that loop for all columns at once, entry position by entry position; col_dots_loop
is the plain Python loop it is checked against).  Maxima do not depend on the order.  Sums are compared with math.fsum
under  2 N 2^-53 sum|terms|  (N terms): recursive summation in ANY order has error <= (N-1)u/(1-(N-1)u) sum|terms|, u = 2^-53,
and the terms themselves are bit-exact, so the factor 2 only covers the denominator.
"""
import math

import numpy as np

U = 2.0 ** -53
TPB, PSTRIDE = 256, 2048                 # workgroup size and grid cap of the vector passes (csrc/solver.hip.hpp)
LONGCOL, LC_CAP, LC_GROUP = 192, 64, 256  # csrc/kernels.hip.hpp
GRID_CAP_LEN = TPB * PSTRIDE             # 524288: longer vectors make a thread loop twice
NSCAL = 11
SUM_SLOTS, MAX_SLOTS = (0, 1, 4, 9, 10), (2, 3, 5, 6, 7, 8)

# pairwise distinct step sizes per candidate, not a 0.75^k ladder: a wrong candidate index or stride changes bits
CAND = dict(tau=(0.37, 0.21, 0.113), theta=(0.9, 0.61, 0.43), bt=(0.5, 0.3125, 0.17), sigma=(0.45, 0.29, 0.19))
COL_LENGTHS = (0, 1, 3, 4, 5, 191, 192, 193, 255, 256, 257, 271, 272, 511, 512, 513, 775, 1024, 5000)


def cand(nc):
    return {k: v[:nc] for k, v in CAND.items()}


# ----------------------------------------------------------------- matrices
def csc_from_lengths(lengths, Q, rng):
    """CSC arrays with the given column lengths: random values, distinct random rows in RANDOM order inside a column."""
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.max(initial=0) <= Q
    colptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    row = np.zeros(colptr[-1], dtype=np.int64)
    for j in np.nonzero(lengths)[0]:
        L = lengths[j]
        row[colptr[j]:colptr[j + 1]] = rng.permutation(Q)[:L] if L > 8 else rng.choice(Q, L, replace=False)
    val = rng.standard_normal(colptr[-1])
    return colptr, row, val


def embed(case, keep):
    """The same problem with empty columns (c = 0) inserted: logical column s becomes column keep[s] of n_wide = the
    case's "n_wide".  The support of the wide problem is exactly `keep`, so blocks of 256 SUPPORT entries are the blocks
    of 256 logical columns."""
    keep = np.asarray(keep, dtype=np.int64)
    nw = int(case["n_wide"])
    lens = np.zeros(nw, dtype=np.int64)
    lens[keep] = np.diff(case["colptr"])
    w = dict(case)
    w["colptr"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rng = np.random.default_rng(99)
    for k in ("x", "x_old", "Mty_old", "c"):
        full = rng.standard_normal(nw) if k != "c" else np.zeros(nw)
        full[keep] = case[k]
        w[k] = full
    w["n"] = nw
    w["keep"] = keep
    return w


def make_case(name, Q, lengths, p, seed, *, c_density=0.5, slack_ineq=False, ties=False, inf_rows=0, roww_zeros=False,
              xold_coef=1.0):
    rng = np.random.default_rng(seed)
    n = len(lengths)
    colptr, row, val = csc_from_lengths(lengths, Q, rng)
    g = lambda k: rng.standard_normal(k)
    cs = dict(name=name, Q=Q, n=n, p=p, colptr=colptr, row=row, val=val, y=g(Q), Mx=g(Q), Mx_old=g(Q), bh=g(Q),
              x=g(n), x_old=g(n), Mty_old=g(n), c=np.where(rng.random(n) < c_density, g(n), 0.0), roww=None,
              xold_coef=xold_coef)
    bh = cs["bh"]
    if slack_ineq:                         # every Mx - h < 0 on the inequality rows
        bh[p:] = cs["Mx"][p:] + rng.uniform(0.5, 2.0, Q - p)
    if ties:                               # ybar / bt == h exactly, for candidate (row mod 3) on every other inequality row
        for i in range(p, Q, 2):
            k = i % 3
            bt, th = CAND["bt"][k], CAND["theta"][k]
            ybar = cs["y"][i] + bt * ((1.0 + th) * cs["Mx"][i] - th * cs["Mx_old"][i])
            bh[i] = ybar / bt
        cs["tie_rows"] = np.arange(p, Q, 2)
    if inf_rows:
        cs["inf_rows"] = p + rng.choice(Q - p, inf_rows, replace=False)
        bh[cs["inf_rows"]] = np.inf
    if roww_zeros:
        cs["roww"] = np.where(rng.random(Q) < 0.3, 0.0, 1.0)
    return cs


def short_lengths(n, rng):
    return rng.integers(0, 6, n)


def small_case(size, pkind):
    """Q = n = size with short columns (at most min(5, Q) entries); pkind 0: p = 0, 1: p = Q, 2: mixed"""
    rng = np.random.default_rng(1000 + size)
    p = (0, size, size // 3)[pkind]
    lens = np.minimum(short_lengths(size, rng), size)
    return make_case(f"small{size}_p{p}", size, lens, p, 2000 + size + pkind)


def special_case(kind):
    Q, n = 300, 130
    rng = np.random.default_rng(7)
    lens = short_lengths(n, rng)
    kw = dict(slack=dict(slack_ineq=True), ties=dict(ties=True), inf=dict(inf_rows=5), roww=dict(roww_zeros=True),
              xold0=dict(xold_coef=0.0), plain=dict())[kind]
    return make_case(f"special_{kind}", Q, lens, 97, 31, **kw)


def column_case():
    """Five and a bit workgroup blocks of 256 columns over Q = 5003 rows:
    block 0: every length class of COL_LENGTHS (12 of them long);  block 1: ONE long column;  block 2: 4;  block 3: 5
    (more than the 4 waves of a workgroup: a wave takes a second column);  block 4: 80 ADJACENT long columns (more than
    LC_CAP = 64: the overflow stays with its threads);  block 5: 77 short columns (n is no multiple of 256)."""
    rng = np.random.default_rng(11)
    n = 5 * 256 + 77
    lens = short_lengths(n, rng)
    slots = rng.permutation(256)[:len(COL_LENGTHS)]
    lens[slots] = COL_LENGTHS
    lens[256 + 100] = 300
    lens[512 + np.array([0, 63, 64, 255])] = (193, 256, 400, 515)
    lens[768 + np.array([1, 2, 130, 200, 254])] = (257, 193, 272, 1030, 200)
    lens[1024 + 90:1024 + 170] = 193 + np.arange(80)
    cs = make_case("columns", 5003, lens, 1700, 12, c_density=2.0)    # (every logical column in the support)
    cs["n_wide"] = n + n // 3 + 1
    return cs


def column_keep(n):
    """logical column s -> wide column: one empty column after every third"""
    s = np.arange(n)
    return s + s // 3


def capped_case():
    """Q = n = 524288 + 257: one more than the 2048 x 256 threads of the capped grid, so threads 0 .. 256 loop twice.  The
    matrix is mostly empty; its long columns sit at indices past 524288, where only the second pass of the grid-stride
    loop finds them.  c is non-zero everywhere, so on the support path |S| = n is past the cap as well."""
    rng = np.random.default_rng(21)
    n = GRID_CAP_LEN + 257
    lens = np.zeros(n, dtype=np.int64)
    some = rng.choice(n, 3000, replace=False)
    lens[some] = rng.integers(1, 6, len(some))
    lens[GRID_CAP_LEN + np.array([3, 100, 101, 256])] = (193, 513, 1024, 300)
    cs = make_case("capped", n, lens, 200000, 22, c_density=2.0)
    assert np.all(cs["c"] != 0.0)
    cs["n_wide"] = n + n // 1000 + 1
    return cs


def capped_keep(n):
    s = np.arange(n)
    return s + s // 1000


def identity_support_cases():
    """c is non-zero in EVERY column, so the support is 0 .. n-1: the support path runs the general path's loops over the
    same entries, through its column map.  Q = n in {1, 64, 65, 257} with short columns, and Q = 300, n = 130 with one column
    just past LONGCOL (193 entries) and one past a round of LC_GROUP (300)."""
    out = []
    for size in (1, 64, 65, 257):
        lens = np.minimum(short_lengths(size, np.random.default_rng(3000 + size)), size)
        out.append(make_case(f"identity{size}", size, lens, size // 3, 4000 + size, c_density=2.0))
    lens = short_lengths(130, np.random.default_rng(17))
    lens[[41, 129]] = (LONGCOL + 1, 300)
    out.append(make_case("identity_long", 300, lens, 97, 4300, c_density=2.0))
    return out


# ----------------------------------------------------------------- references
def col_dots_loop(colptr, row, val, y, cols=None):
    """the specification: one sequential float64 accumulation per column, in storage order"""
    out = {}
    for j in (range(len(colptr) - 1) if cols is None else cols):
        acc = 0.0
        for k in range(colptr[j], colptr[j + 1]):
            acc += float(val[k]) * float(y[row[k]])
        out[j] = acc
    return out


def col_dots(colptr, row, val, Y):
    """the same loop for every column and every row of Y (nc x Q) at once: step t adds entry t of every column that has one"""
    Y = np.atleast_2d(Y)
    n = len(colptr) - 1
    lens = np.diff(colptr)
    order = np.argsort(-lens, kind="stable")
    sl, start = lens[order], colptr[:-1][order]
    acc = np.zeros((Y.shape[0], n))
    for t in range(int(sl[0]) if n else 0):
        m = int(np.searchsorted(-sl, -t, side="left"))            # columns longer than t
        k = start[:m] + t
        acc[:, order[:m]] += val[k] * Y[:, row[k]]
    return acc


def support_of(cs):
    return np.nonzero((np.diff(cs["colptr"]) > 0) | (cs["c"] != 0.0))[0]


def sum_bound(terms):
    terms = np.asarray(terms, dtype=np.float64)
    return 2.0 * len(terms) * U * math.fsum(np.abs(terms))


def reference(cs, nc=3, plain=False, support=False, c0=-1, tau_re=0.0, sigma_re=0.0, tau_update=0.0):
    """Everything proxsdp_hip_trial_batch returns, from the reference's expressions.  For every candidate: y, Mty, the six
    maxima (dict slot -> value) and the terms of the five sums (dict slot -> array)."""
    Q, n, p = cs["Q"], cs["n"], cs["p"]
    y0, Mx, Mx_old, bh = cs["y"], cs["Mx"], cs["Mx_old"], cs["bh"]
    roww = cs["roww"] if cs["roww"] is not None else np.ones(Q)
    wres = roww if support else np.ones(Q)          # the general path's residual pass takes no row weights
    S = support_of(cs) if support else np.arange(n)
    x, xo, mo, cv = cs["x"][S], cs["x_old"][S], cs["Mty_old"][S], cs["c"][S]
    K = cand(nc)
    ref = dict(S=S, y=np.zeros((nc, Q)), Mty=np.zeros((nc, len(S))), maxs=[], sums=[])
    dys = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(nc):
            bt, th = K["bt"][k], K["theta"][k]
            ybar = y0 + bt * ((1.0 + th) * Mx - th * Mx_old)
            proj = bh.copy()
            proj[p:] = np.minimum(ybar[p:] / bt, bh[p:])
            yn = ybar - bt * proj
            d = yn - y0
            dys.append(d)
            ref["y"][k] = yn if plain else d + y0
        acc = col_dots(cs["colptr"], cs["row"], cs["val"], ref["y"])[:, S]
        dm = acc - mo
        ref["Mty"][:] = acc if plain else dm + mo

        def residual(k, yk, mk, tau, sigma):
            pold = cs["xold_coef"] * xo - tau * mo
            pnew = x - tau * mk
            qold = y0 - sigma * Mx_old
            qnew = yk - sigma * Mx
            z = lambda a: float(np.max(a, initial=0.0))
            maxs = {2: z(np.abs(pnew - pold)), 3: z(np.abs(pold)), 5: z(np.abs(qnew - qold)), 6: z(np.abs(qold)),
                    7: z(np.abs(Mx[:p] - bh[:p])), 8: z(Mx[p:] - bh[p:])}
            sums = {4: cv * x, 9: wres[:p] * (bh[:p] * yk[:p]), 10: wres[p:] * (bh[p:] * yk[p:])}
            return maxs, sums
        for k in range(nc):
            maxs, sums = residual(k, ref["y"][k], ref["Mty"][k], K["tau"][k], K["sigma"][k])
            dk = dys[k]
            sums[0] = roww * (dk * dk)
            sums[1] = dm[k] * dm[k]
            ref["maxs"].append(maxs)
            ref["sums"].append(sums)
        if c0 >= 0:
            ref["re"] = residual(c0, ref["y"][c0], ref["Mty"][c0], tau_re, sigma_re)
        if support:                                             # k_primal_update_S on x_old with M'y = Mty_old
            upd = tau_update * (mo + cv)
            xn = xo - upd
            xu = cs["x_old"].copy()
            xu[S] = xn
            ref.update(x_upd=xu, xsave=xo.copy(), esv=np.stack([-upd, xn]))
    return ref


def hook_args(cs, nc=3, plain=False, support=False, c0=-1, tau_re=0.0, sigma_re=0.0, tau_update=0.0):
    """keyword arguments of binding.trial_batch for this case"""
    K = cand(nc)
    return dict(p=cs["p"], bh=cs["bh"], y=cs["y"], Mx=cs["Mx"], Mx_old=cs["Mx_old"], x=cs["x"], x_old=cs["x_old"],
                Mty_old=cs["Mty_old"], c=cs["c"], roww=cs["roww"], xold_coef=cs["xold_coef"], support=support, plain=plain,
                c0=c0, tau_re=tau_re, sigma_re=sigma_re, tau_update=tau_update, **K)


# ----------------------------------------------------------------- second-order cones and 1x1 blocks
SOC_LENGTHS = (1, 2, 3, 64, 255, 256, 257, 1025, 100000)


def soc_bound(length, s, nv):
    """per-entry tolerance of a projected cone: a sum of len non-negative squares has relative error <= (len + 1) u, the
    square root halves it and adds u, val = 0.5 (1 + s / nv) adds three roundings, the final product one more:
    (len + 8) u max(|s|, nv) covers it"""
    return (length + 8) * U * max(abs(float(s)), float(nv))


def soc_cases():
    """(name, branch, vector) with vector[0] = s.  Branch: 'polar' (nv <= -s: all zeros), 'inside' (nv <= s: unchanged),
    'outside' (scaled).  Ties come from exactly representable data; the others are separated by far more than 1e-6 nv."""
    rng = np.random.default_rng(5)
    out = [("tie_3_4_5", "inside", np.array([5.0, 3.0, 4.0])),
           ("tie_3_4_m5", "polar", np.array([-5.0, 3.0, 4.0])),
           ("tie_3_m4_m5", "polar", np.array([-5.0, 3.0, -4.0])),     # (scaling by val = 0 instead would leave a -0.0)
           ("tie_zero_tail_s0", "polar", np.array([0.0, 0.0, 0.0])),
           ("tie_zero_tail_negzero", "polar", np.array([-0.0, 0.0, 0.0])),
           ("len1_pos", "inside", np.array([2.5])),
           ("len1_neg", "polar", np.array([-2.5])),
           ("len1_negzero", "polar", np.array([-0.0])),
           ("len2_outside", "outside", np.array([1.0, 3.0])),
           ("len2_inside", "inside", np.array([3.0, -1.0])),
           ("len2_polar", "polar", np.array([-3.0, 1.0]))]
    for L in SOC_LENGTHS[2:]:
        for branch, f in (("outside", 0.3), ("outside", -0.4), ("inside", 1.5), ("polar", -1.7)):
            if L == 100000 and f == -0.4:
                continue
            v = rng.standard_normal(L)
            v[0] = f * float(np.sqrt(np.sum(v[1:] * v[1:])))
            out.append((f"len{L}_{branch}_{f}", branch, v))
    return out


def soc_layout():
    """All cones in ONE vector at non-contiguous offsets, in an order unrelated to the cone index, with sentinel entries in
    the gaps; the 1x1 blocks sit on gap entries.  Returns x, soc_off, soc_len, one_off, and the cases in cone order."""
    cases = soc_cases()
    rng = np.random.default_rng(6)
    place = rng.permutation(len(cases))                # memory order of the cones
    off = np.zeros(len(cases), dtype=np.int64)
    chunks, gaps, pos = [], [], 0
    for ci in place:
        g = int(rng.integers(1, 8))
        chunks.append(rng.standard_normal(g))
        gaps.extend(range(pos, pos + g))
        pos += g
        off[ci] = pos
        chunks.append(cases[ci][2])
        pos += len(cases[ci][2])
    chunks.append(rng.standard_normal(3))
    gaps.extend(range(pos, pos + 3))
    x = np.concatenate(chunks)
    one_off = rng.choice(np.array(gaps), 24, replace=False)
    x[one_off] = np.resize(np.array([-1.5, 0.0, -0.0, 2.25, -1e-300, 1e-300]), 24)
    return x, off, np.array([len(c[2]) for c in cases], dtype=np.int32), one_off, cases


def soc_reference(v):
    """longdouble restatement of soc_projection! (prox_operators.jl:145-158): (branch, projected vector, nv, gap = nv - s)"""
    w = np.asarray(v, dtype=np.longdouble)
    s = w[0]
    nv = np.sqrt(np.sum(w[1:] * w[1:]))
    if nv <= -s:
        return "polar", np.zeros_like(w), nv, nv - s
    if nv <= s:
        return "inside", w.copy(), nv, nv - s
    val = np.longdouble(0.5) * (1 + s / nv)
    out = w * val
    out[0] = val * nv
    return "outside", out, nv, nv - s


def soc_numpy(v):
    """the same in float64 NumPy (pairwise sum of squares)"""
    v = np.asarray(v, dtype=np.float64)
    s = v[0]
    nv = np.sqrt(np.sum(v[1:] * v[1:]))
    if nv <= -s:
        return np.zeros_like(v)
    if nv <= s:
        return v.copy()
    val = 0.5 * (1.0 + s / nv)
    out = v * val
    out[0] = val * nv
    return out
