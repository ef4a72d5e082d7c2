"""What the certified dual bound of a kept model costs and loses: writes profiles/dual_bound.md.

Max-Cut on G(n, p), average degree 12, seed 0, reference default options, n = 4000 (and any other `--sizes`): one default
solve on a kept model, then `Model.bound` from that solution's duals, in one session on one otherwise idle GPU.

    call        proxsdp_dual_bound.seconds and the wall time Python sees, median of `--runs` calls after one warm-up call
    tries       factorisations of the shift search; how many completed and how many failed follows from sigma* (a try
                completed exactly when its shift was >= sigma*: the search is replayed here)
    completed   the time of ONE completed factorisation: factor_seconds of a call whose duals are shifted until Z~ is
                clearly positive definite (one try, sigma = 0, the flag read-back included)
    failed      the mean time of a failed try in the call on the solution's duals: (factor_seconds - completed tries x
                completed) / failed tries; a failed try ends at its first bad pivot, every later launch returns at once
    loss        T (sigma* + delta + rho): what the certificate costs beside the ideal bound of the same duals, beside
                |objval - dual_objval| of the solve
    torch       torch.linalg.cholesky_ex on the same dense matrix Z~ + sigma* I on the same device: the thing to compare one
                completed factorisation with (the parent has no counterpart)

Recorded, not asserted.

    python tools/measure_dual_bound.py [--sizes 4000] [--runs 3] [--out profiles/dual_bound.md]
"""
import argparse
import math
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent


def replay(nu, sigma_star):
    """(completed, failed) tries of the shift search when a try completes exactly for sigma >= sigma_star"""
    done = fail = 0
    ok = lambda s: s >= sigma_star
    if ok(0.0):
        return 1, 0
    fail += 1
    lo = 0.0
    for j in range(13):
        s = math.ldexp(nu, -48 + 4 * j)
        if ok(s):
            done += 1
            hi = s
            if j >= 1:
                for _ in range(5):
                    mid = math.sqrt(lo) * math.sqrt(hi)
                    if ok(mid):
                        done += 1; hi = mid
                    else:
                        fail += 1; lo = mid
            return done, fail
        fail += 1
        lo = s
    return done, fail


def measure(sizes, runs):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import numpy as np
    import torch                                      # (before the library loads: binding.lib)
    from proxsdp_jl_amd import binding as B
    from proxsdp_jl_amd import problems as P
    import bound_cases as K
    if B.device_count() <= 0:
        raise SystemExit("needs a HIP device")
    sync = torch.cuda.synchronize

    def clock(call):
        sync()
        t0 = time.perf_counter()
        out = call()
        sync()
        return out, time.perf_counter() - t0

    B.solve(P.maxcut(150, seed=0), B.default_options(), device_out=True)      # (loads the code objects)
    res = {}
    for n in sizes:
        pr = P.maxcut(n, seed=0)
        mdl = B.Model(pr, B.default_options())
        sol, t_solve = clock(lambda: mdl.solve())
        ye, yi = np.asarray(sol.dual_eq), np.asarray(sol.dual_in)
        Zt = K.dual_matrices(pr, ye, yi)[0]
        nu = float(np.abs(Zt).sum(axis=1).max())
        walls, recs = [], []
        for k in range(runs + 1):
            db, t = clock(lambda: mdl.bound((ye, yi)))
            if k:
                walls.append(t); recs.append(db)
        med = lambda f: statistics.median(f(r) for r in recs)
        one = [mdl.bound((ye + 2.0 * nu, yi)) for _ in range(runs + 1)][1:]       # Z~ + 2 nu I: sigma = 0 completes
        assert all(r.factorisations[0] == 1 and r.shift[0] == 0.0 for r in one)
        t_done = statistics.median(r.factor_seconds for r in one)
        n_done, n_fail = replay(nu, float(db.shift[0]))
        if n_done + n_fail != int(db.factorisations[0]):                           # (a try near the threshold went the other way)
            n_done, n_fail = 1, int(db.factorisations[0]) - 1
        t_fail = (med(lambda r: r.factor_seconds) - n_done * t_done) / n_fail if n_fail else float("nan")
        Zd = torch.as_tensor(Zt + float(db.shift[0]) * np.eye(n), device="cuda:0")
        t_torch = []
        for k in range(runs + 1):
            (_, info), t = clock(lambda: torch.linalg.cholesky_ex(Zd))
            if k:
                t_torch.append(t)
        res[n] = dict(iter=int(sol.iter), solve=t_solve, objval=pr.user_objective(sol.objval), dual_objval=pr.user_objective(sol.dual_objval),
                      dual_feas=float(sol.dual_feasibility), bound=pr.user_objective(db.bound), tries=int(db.factorisations[0]),
                      done=n_done, fail=n_fail, call=med(lambda r: r.seconds), wall=statistics.median(walls),
                      factor=med(lambda r: r.factor_seconds), t_done=t_done, t_fail=t_fail, shift=float(db.shift[0]),
                      delta=float(db.delta[0]), rho=float(db.radius[0]), loss=db.loss, lam=float(np.linalg.eigvalsh(Zt).min()),
                      allocated=db.bytes_allocated, torch=statistics.median(t_torch), torch_info=int(info))
        mdl.close()
        print(n, res[n], flush=True)
    return res


def report(res, runs, out):
    lines = ["# A certified dual bound of a kept model by a device Cholesky test (tools/measure_dual_bound.py)", "",
             "Max-Cut, G(n, p) with average degree 12, seed 0; reference default options; one MI355X, otherwise idle.  One",
             "default solve on a kept model, then `Model.bound` from its duals (host arrays).  Seconds; `call`",
             f"(proxsdp_dual_bound.seconds), `wall` and `factor` (factor_seconds) are medians of {runs} calls after one warm-up",
             "call.  `completed` = one completed factorisation (a call whose duals make Z~ clearly positive definite: one try,",
             "the flag read-back included); `failed` = the mean failed try of the call on the solution's duals (it ends at the",
             "first bad pivot).  `torch` = `torch.linalg.cholesky_ex` on the same dense Z~ + sigma* I on the same device.",
             "Objective values and the bound are in the user's sense (maximisation: the bound is an UPPER bound).", "",
             "| n | tries | completed / failed | call | wall | factor | completed | failed | torch | completed / torch | scratch, MiB |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in sorted(res):
        r = res[n]
        lines.append("| %d | %d | %d / %d | %.4f | %.4f | %.4f | %.5f | %.5f | %.5f | %.2f | %.1f |" % (
            n, r["tries"], r["done"], r["fail"], r["call"], r["wall"], r["factor"], r["t_done"], r["t_fail"], r["torch"],
            r["t_done"] / r["torch"], r["allocated"] / 2.0 ** 20))
    lines += ["", "| n | objval | dual_objval | objval - dual_objval | dual_feasibility | lambda_min(Z~) (NumPy) | sigma* | delta | rho | loss T (sigma* + delta + rho) | certified bound |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in sorted(res):
        r = res[n]
        lines.append("| %d | %.6f | %.6f | %.3g | %.3g | %.6g | %.6g | %.3g | %.3g | %.6g | %.6f |" % (
            n, r["objval"], r["dual_objval"], abs(r["objval"] - r["dual_objval"]), r["dual_feas"], r["lam"], r["shift"], r["delta"],
            r["rho"], r["loss"], r["bound"]))
    lines += ["", "Solves: " + ", ".join("n = %d: %d iterations, %.2f s" % (n, res[n]["iter"], res[n]["solve"]) for n in sorted(res)) +
              ".  torch's factorisation reported info = " + ", ".join(str(res[n]["torch_info"]) for n in sorted(res)) + "."]
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4000])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dual_bound.md"))
    a = ap.parse_args()
    report(measure(a.sizes, a.runs), a.runs, a.out)


if __name__ == "__main__":
    main()
