"""What a warm start (proxsdp_hip_solve_from) is worth on the GPU: writes profiles/warm_start.md.

Max-Cut on G(n, p) graphs (problems.maxcut, seed 0), reference default options, n = 1000 and n = 4000:
  cold                     the plain solve, its factors kept (solve(factors=True))
  warm, own factors        the same model started from that result (factors + duals; target rank = rank + 1)
  perturbed, cold          every edge weight multiplied by 1 + 0.01 N(0, 1), solved cold
  perturbed, warm          the perturbed model started from the UNPERTURBED solution
and, at the largest size, the set-up cost of the two ways to hand over the same point: factors (8 n r bytes, rebuilt by
the reconstruction kernel) against the dense primal (the packed triangle, gathered by k_start_gather) with the factored
run's target rank.  Recorded, not asserted.

    python tools/measure_warm_start.py [--sizes 1000 4000] [--out profiles/warm_start.md]
"""
import argparse
import pathlib
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from proxsdp_jl_amd import binding as B          # noqa: E402
from proxsdp_jl_amd import problems as P         # noqa: E402


def perturbed_laplacian(L, seed, rel=0.01):
    """the Laplacian of the same graph with every edge weight multiplied by 1 + rel N(0, 1)"""
    W = sp.triu(-sp.coo_matrix(L), k=1).tocoo()
    rng = np.random.default_rng(seed)
    w = W.data * (1.0 + rel * rng.standard_normal(len(W.data)))
    W = sp.coo_matrix((w, (W.row, W.col)), shape=L.shape)
    W = (W + W.T).tocsr()
    return (sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()


def solve(pr, **kw):
    t0 = time.time()
    sol = B.solve(pr, B.default_options(), **kw)
    sol.wall = time.time() - t0
    return sol


def row(label, n, sol):
    r = sol.psd_factors[0][2]["rank_found"] if getattr(sol, "psd_factors", None) else sol.final_rank
    return "| %d | %s | %d | %d | %d | %.3f | %.3f | %.3f | %.9g |" % (
        n, label, sol.status, sol.iter, r, sol.stats["loop_time"], sol.stats["init_time"], sol.wall, -sol.objval)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4000])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "warm_start.md"))
    a = ap.parse_args()
    if B.device_count() <= 0:
        raise SystemExit("needs a HIP device")
    solve(P.maxcut(150, seed=0))                      # (loads the code objects: keeps that out of the first row's init_time)
    lines = ["# Warm start on the GPU (tools/measure_warm_start.py)", "",
             "Max-Cut, G(n, p) with average degree 12, seed 0; reference default options; one MI355X.  `status` 1 = OPTIMAL.",
             "`loop` and `init` are the library's own timers (stats.loop_time, stats.init_time: preprocess + upload + the start",
             "path), `wall` the whole call seen from Python (marshalling and the exit path included).", "",
             "| n | run | status | iterations | rank | loop s | init s | wall s | objective |",
             "|---|---|---|---|---|---|---|---|---|"]
    extra = []
    for n in a.sizes:
        L = P.erdos_renyi_laplacian(n, 0)
        pr = P.maxcut_from_laplacian(L, name=f"maxcut-{n}")
        prp = P.maxcut_from_laplacian(perturbed_laplacian(L, 1), name=f"maxcut-{n}-perturbed")
        cold = solve(pr, factors=True)
        lines.append(row("cold", n, cold)); print(lines[-1], flush=True)
        warm = solve(pr, factors=True, start=cold)
        lines.append(row("warm, own factors + duals", n, warm)); print(lines[-1], flush=True)
        pcold = solve(prp, factors=True)
        lines.append(row("perturbed 1 %, cold", n, pcold)); print(lines[-1], flush=True)
        pwarm = solve(prp, factors=True, start=cold)
        lines.append(row("perturbed 1 %, warm from the unperturbed solution", n, pwarm)); print(lines[-1], flush=True)
        if n == max(a.sizes):
            rank = cold.psd_factors[0][2]["rank_found"]
            dense = solve(pr, start=dict(primal=cold.primal, dual_eq=cold.dual_eq, dual_in=cold.dual_in, target_rank=[rank + 1]))
            fact = solve(pr, start=cold)
            extra = ["", "## Handing over the same point: factors against the dense primal (n = %d, rank %d)" % (n, rank), "",
                     "| start | bytes handed over for the PSD block | init s | iterations | loop s | wall s |", "|---|---|---|---|---|---|",
                     "| factors `V`, `λ` | %d | %.3f | %d | %.3f | %.3f |" % (8 * n * rank + 8 * rank, fact.stats["init_time"], fact.iter, fact.stats["loop_time"], fact.wall),
                     "| dense `primal`, explicit target rank | %d | %.3f | %d | %.3f | %.3f |" % (8 * pr.n, dense.stats["init_time"], dense.iter, dense.stats["loop_time"], dense.wall),
                     "| (cold, for scale) | 0 | %.3f | %d | %.3f | %.3f |" % (cold.stats["init_time"], cold.iter, cold.stats["loop_time"], cold.wall)]
            for ln in extra:
                print(ln, flush=True)
    pathlib.Path(a.out).write_text("\n".join(lines + extra) + "\n")


if __name__ == "__main__":
    main()
