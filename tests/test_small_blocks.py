"""The one-launch small-block projections (k_small_psd_project: cyclic Jacobi in LDS; k_small_sign_project: the sign iteration
in LDS) AS THE SOLVER LAUNCHES THEM: proxsdp_hip_project_cones runs setup_device, classify_blocks, setup_small_batch, setup_soc,
psd_projection at iteration 1 and harvest_small_ranks on a vector of mixed cones -- the mixed-side grid with its LDS grant,
the nmin / nmax hand-over between the two kernels, the rank record on both of its routes, the -1 record.

Every block is compared with Q diag(max(w, 0)) Q' evaluated in longdouble (tests/small_block_cases.py; the reference's own error
is below 1e-15 x the spectral scale, test_small_blocks_host.py).  Tolerances: Jacobi blocks 1e-13 x scale, sign blocks and the
blocks of the per-block engines 1e-10 x scale (the contract stated in small_sign.hip.hpp; the LAPACK-accurate engines lie
within it).  Each test prints its worst error-to-tolerance ratio per engine and side.

Sweep counts: the device's count on a Jacobi block must be <= s_ref + 2, s_ref from the NumPy restatement of the schedule
(small_block_cases.restated_jacobi), never from the kernel; the margin allows for the device's summation order in off^2.
"""
import numpy as np
import pytest

import small_block_cases as SC
from proxsdp_jl_amd import binding as B

pytestmark = pytest.mark.gpu

TOL = {"small-jacobi": 1e-13, "small-sign": 1e-10, "large": 1e-10}
BIG = [i for i, s in enumerate(SC.SIDES) if s > 1]


def _classes(jacobi, sign):
    """expected class per block: sides in `jacobi` / `sign` (inclusive ranges) are small, side 1 is 1x1, the rest large"""
    def cls(s):
        if s == 1:
            return "1x1"
        if jacobi and jacobi[0] <= s <= jacobi[1]:
            return "small-jacobi"
        if sign and sign[0] <= s <= sign[1]:
            return "small-sign"
        return "large"
    return [cls(s) for s in SC.SIDES]


# name -> (options, expected classes, sides of the large blocks the tiled sign projection serves, shortened sign schedule?)
OPTION_SETS = {
    "default": (dict(), _classes((2, 2), (3, 64)), (65,), True),
    "jacobi": (dict(small_block_batch=1), _classes((2, 64), None), (65,), True),
    "sign": (dict(small_block_batch=2), _classes(None, (2, 64)), (65,), True),
    "tight": (dict(tol_gap=1e-9), _classes((2, 32), None), (), True),
    "off": (dict(small_block_batch=0), _classes(None, None), (33, 48, 64, 65), True),
    "sign_full_table": (dict(small_block_batch=2, sign_start_row=0), _classes(None, (2, 64)), (65,), False),
}


def _options(kw):
    o = B.default_options()
    for k, v in kw.items():
        B.set_option(o, k, v)
    return o


@pytest.fixture(scope="module")
def problems():
    return {layout: SC.problem(layout) for layout in SC.LAYOUTS}


def _project(problems, layout, kw, d, swap=False):
    """one call; a non-finite error is allowed only to a deal that holds a 2^+520 block: the call is then made once more
    with those blocks' unscaled data, and must succeed.  Returns (x, cases, result, replaced block indices)"""
    x, cases = SC.vector(layout, d, swap)
    try:
        return x, cases, B.project_cones(problems[layout], x, _options(kw)), ()
    except B.ProxSDPHipError as e:
        huge = {i: c.base for i, c in enumerate(cases) if c is not None and c.kind == "huge"}
        assert e.code == -2 and "non-finite" in str(e) and huge, (layout, kw, d, str(e))
    x, cases = SC.vector(layout, d, swap, replace=huge)
    return x, cases, B.project_cones(problems[layout], x, _options(kw)), tuple(huge)


class Ratios:
    """worst error-to-tolerance ratio per (engine, side)"""

    def __init__(self):
        self.worst = {}

    def add(self, cls, side, ratio, kind):
        key = (cls, side)
        if ratio >= self.worst.get(key, (-1.0, ""))[0]:
            self.worst[key] = (ratio, kind)

    def show(self, title):
        print(f"\n[{title}] worst error / tolerance per engine and side")
        for (cls, side), (r, kind) in sorted(self.worst.items()):
            print(f"  {cls:13s} side {side:2d}: {r:9.3e}  ({kind})")


def _check(name, layout, d, x, cases, res, ratios, sweeps_log=None):
    kw, classes, tiled, short = OPTION_SETS[name]
    offs, sides, (so, sl), fo, n = SC.block_table(SC.LAYOUTS[layout])
    assert list(res["offset"]) == offs and list(res["side"]) == sides
    assert res["cls"] == classes, (name, res["cls"])
    st = res["stats"]
    n_small = sum(c.startswith("small") for c in classes)
    n_sign = classes.count("small-sign")
    assert st["batched_small_eigs"] == n_small
    assert st["full_eigs"] == len(BIG)
    assert st["full_eigs_sign"] == n_sign + len(tiled)
    assert st["sign_short_pass"] + st["sign_short_fail"] == (n_sign + len(tiled) if short else 0)
    # everything outside the PSD blocks comes back bit for bit
    assert np.array_equal(res["x"][so:], x[so:])
    ones = iter(SC.one_by_one(d))
    for i, (o, s, c, cls) in enumerate(zip(offs, sides, cases, classes)):
        got = res["x"][o:o + SC.packed_len(s)]
        if s == 1:
            v = max(0.0, next(ones))
            assert got[0] == v and res["min_eig"][i] == v and res["rank"][i] == 0 and res["sweeps"][i] == -1
            continue
        err = float(np.abs(SC.smat_ld(got, s) - c.ref).max())
        tol = TOL[cls] * c.scale
        ratio = err / tol if tol > 0 else (0.0 if err == 0.0 else np.inf)
        ratios.add(cls, s, ratio, c.kind)
        assert err <= tol, (name, layout, d, cls, s, c.kind, err / max(c.scale, 1e-300))
        rank = int(res["rank"][i])
        if cls == "small-jacobi":
            assert rank == c.rank, (name, d, s, c.kind, rank, c.rank)
            sw = int(res["sweeps"][i])
            if sweeps_log is not None:
                sweeps_log.append((s, c.kind, sw, c.s_ref))
            assert (sw == 0) if c.degenerate else (0 < sw <= c.s_ref + 2), (name, d, s, c.kind, sw, c.s_ref)
        else:
            assert res["sweeps"][i] == -1
        if cls == "small-sign" or (cls == "large" and s in tiled):
            assert c.npos <= rank <= c.npos + c.nzero, (name, d, s, c.kind, rank, c.npos, c.nzero)
        if cls.startswith("small"):
            assert res["min_eig"][i] == 0.0


@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_every_block_of_both_layouts_against_the_longdouble_reference(name, problems):
    """classes, values, ranks, 1x1 blocks, counters, untouched entries -- every deal on both layouts; the padded layout
    (P.n > 65536: the rank record goes through the device buffer and one copy) must give the mixed layout's bits"""
    kw = OPTION_SETS[name][0]
    ratios, sweeps_log = Ratios(), []
    for d in range(SC.DEALS):
        xm, cm, rm, rep_m = _project(problems, "mixed", kw, d)
        _check(name, "mixed", d, xm, cm, rm, ratios, sweeps_log)
        xp, cp, rp, rep_p = _project(problems, "padded", kw, d)
        _check(name, "padded", d, xp, cp, rp, ratios)
        assert rep_m == rep_p
        assert np.array_equal(rm["x"], rp["x"][:len(xm)])
        for f in ("rank", "min_eig", "sweeps"):
            assert np.array_equal(rm[f], rp[f]), f
        assert rm["cls"] == rp["cls"] and rm["stats"] == rp["stats"]
        if rep_m:
            print(f"[{name}] deal {d}: 2^+520 block(s) {[SC.SIDES[i] for i in rep_m]} answered by the non-finite error")
    ratios.show(name)
    if sweeps_log:
        by_side = {}
        for s, kind, sw, sref in sweeps_log:
            by_side.setdefault(s, []).append(f"{kind} {sw}/{sref}")
        print(f"[{name}] Jacobi sweeps, device / s_ref:")
        for s in sorted(by_side):
            print(f"  side {s:2d}: " + ", ".join(by_side[s]))


@pytest.mark.parametrize("name", ["default", "jacobi", "sign"])
def test_repeatable_and_each_block_follows_its_data(name, problems):
    """two calls give identical bits; with the first and the last block of side 2 trading their data, each of the two results
    follows its data and every other block keeps its bits"""
    kw = OPTION_SETS[name][0]
    offs, sides, _, _, _ = SC.block_table(SC.LAYOUTS["mixed"])
    twos = [i for i, s in enumerate(sides) if s == 2]
    a, b = twos[0], twos[-1]
    ratios = Ratios()
    for d in (0, 3, 7):
        x, cases, r1, rep = _project(problems, "mixed", kw, d)
        r2 = B.project_cones(problems["mixed"], x, _options(kw))
        assert np.array_equal(r1["x"], r2["x"]) and all(np.array_equal(r1[f], r2[f]) for f in ("rank", "min_eig", "sweeps"))
        assert r1["stats"] == r2["stats"]
        xs, cs, rs, rep_s = _project(problems, "mixed", kw, d, swap=True)
        assert rep == rep_s and cs[a] is cases[b] and cs[b] is cases[a]
        _check(name, "mixed", d, xs, cs, rs, ratios)
        sl = lambda r, i: r["x"][offs[i]:offs[i] + 3]
        assert np.array_equal(sl(rs, a), sl(r1, b)) and np.array_equal(sl(rs, b), sl(r1, a))
        for f in ("rank", "sweeps"):
            assert rs[f][a] == r1[f][b] and rs[f][b] == r1[f][a]
        keep = np.ones(len(x), dtype=bool)
        keep[offs[a]:offs[a] + 3] = False
        keep[offs[b]:offs[b] + 3] = False
        assert np.array_equal(rs["x"][keep], r1["x"][keep])


@pytest.mark.parametrize("side", [2, 17])
def test_non_finite_input_is_the_librarys_error(side, problems):
    """one NaN in a Jacobi block (side 2) / a sign block (side 17) under the default options: the -1 rank record makes
    harvest_small_ranks throw, and the call comes back with the library's error -- one call each; the library works afterwards"""
    x, cases = SC.vector("mixed", 0)
    offs, sides, _, _, _ = SC.block_table(SC.LAYOUTS["mixed"])
    i = sides.index(side)
    assert OPTION_SETS["default"][1][i] == ("small-jacobi" if side == 2 else "small-sign")
    x[offs[i] + 1] = np.nan
    with pytest.raises(B.ProxSDPHipError) as ei:
        B.project_cones(problems["mixed"], x, _options({}))
    assert ei.value.code == -2 and "non-finite" in str(ei.value)
    x, cases = SC.vector("mixed", 1)
    _check("default", "mixed", 1, x, cases, B.project_cones(problems["mixed"], x, _options({})), Ratios())
