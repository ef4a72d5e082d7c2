"""What the pentagonal / heptagonal separation on the device costs and finds: writes profiles/clique_cuts.md.

The instance of profiles/triangle_cuts.md -- Max-Cut on G(n, p), average degree 12, seed 0, reference default options -- at
n = 1000 and n = 4000.  One cold solve on a kept model (vectors on the device) gives the first solution; its `--bases` most
violated triangle rows (Model.separate_triangles) are the bases.  On that solution, in one session on one otherwise idle GPU:

    q = 3      Model.separate_cliques(first, triangles): every base against all 4 C(n - 3, 2) pairs and signs
    q = 5      Model.separate_cliques(first, those pentagons): the same one size up
    torch      the same extension written in torch on the device, batched over as many bases as fit in `--torch-gib` of
               temporaries: what a user would write today (first maximum per base; no merge, no rows)

    wall       the call as Python sees it (device synchronised), median of `--runs` calls after one warm-up call
    library    proxsdp_clique_cuts.seconds
    sweep      proxsdp_clique_cuts.sweep_seconds: the sweep kernels alone, between device events, summed over the batches
    rate       scanned / sweep, evaluations per second; beside it the triangle sweep's (scanned / sweep_seconds of
               Model.separate_triangles) measured in the same session

and one full round at the largest size -- separate (q = 3), Model.change_rows(add=...), Model.solve(start=change.carry(first))
-- with the objective before and after it.

Recorded, not asserted.

    python tools/measure_clique_cuts.py [--sizes 1000 4000] [--runs 5] [--bases 1000] [--out profiles/clique_cuts.md]
"""
import argparse
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
CODES = ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0))


def torch_extend(torch, X, nodes, signs, rhs, gib):
    """(v, l, m, code) per base: the contract's value over all pairs and codes as whole tensors, chunks of bases at a time"""
    s, (nb, q) = X.shape[0], nodes.shape
    chunk = max(1, int(gib * 2.0 ** 30 / (8.0 * s * s * 3)))
    lower = torch.tril(torch.ones(s, s, dtype=torch.bool, device=X.device))
    out = []
    for c0 in range(0, nb, chunk):
        a, sg = nodes[c0:c0 + chunk], signs[c0:c0 + chunk]
        t = (sg[:, :, None] * X[a]).sum(1)
        t.scatter_(1, a, float("nan"))
        B = torch.zeros(len(a), dtype=X.dtype, device=X.device)
        for u in range(q):
            for w in range(u + 1, q):
                B = B + (-sg[:, u] * sg[:, w]) * X[a[:, u], a[:, w]]
        best = None
        for code, (tl, tm) in enumerate(CODES):
            V = B[:, None, None] - tl * t[:, :, None] - tm * t[:, None, :] - (tl * tm) * X[None] - rhs
            V = torch.where(lower[None] | torch.isnan(V), torch.full_like(V, float("-inf")), V)
            v, arg = V.reshape(len(a), -1).max(1)
            if best is None:
                best = (v, arg, torch.zeros_like(arg))
            else:
                take = v > best[0]
                best = (torch.where(take, v, best[0]), torch.where(take, arg, best[1]), torch.where(take, torch.full_like(arg, code), best[2]))
        out.append(best)
    v, arg, code = (torch.cat([o[k] for o in out]) for k in range(3))
    return v, arg // s, arg % s, code


def measure(sizes, runs, nbases, gib):
    sys.path.insert(0, str(ROOT))
    import numpy as np
    import torch                                      # (before the library loads: binding.lib)
    from proxsdp_jl_amd import binding as B
    from proxsdp_jl_amd import problems as P
    if B.device_count() <= 0:
        raise SystemExit("needs a HIP device")
    sync = torch.cuda.synchronize

    def clock(call):
        sync()
        t0 = time.perf_counter()
        out = call()
        sync()
        return out, time.perf_counter() - t0

    def timed(call, reps):
        recs = []
        for k in range(reps + 1):
            out, t = clock(call)
            if k:
                recs.append((t, out))
        return recs

    B.solve(P.maxcut(150, seed=0), B.default_options(), device_out=True)      # (loads the code objects)
    res = {}
    for n in sizes:
        pr = P.maxcut(n, seed=0)
        mdl = B.Model(pr, B.default_options())
        first, t_first = clock(lambda: mdl.solve(device_out=True))
        tri = [c for _, c in timed(lambda: mdl.separate_triangles(first, count=nbases), runs)]
        tri_rate = statistics.median(c.scanned / c.sweep_seconds for c in tri)
        r = dict(first_iter=int(first.iter), first_objval=float(first.objval), first_wall=t_first, tri_rate=tri_rate,
                 tri_sweep=statistics.median(c.sweep_seconds for c in tri))
        bases = tri[-1]
        X = torch.zeros(n, n, dtype=torch.float64, device="cuda:0")
        jj, ii = np.repeat(np.arange(n), np.arange(1, n + 1)), np.concatenate([np.arange(j + 1) for j in range(n)])
        packed = first.primal[torch.as_tensor(pr.psd[0], device="cuda:0")]
        ii, jj = torch.as_tensor(ii, device="cuda:0"), torch.as_tensor(jj, device="cuda:0")
        X[ii, jj] = packed
        X[jj, ii] = packed
        for q in (3, 5):
            recs = timed(lambda: mdl.separate_cliques(first, bases), runs)
            cuts = recs[-1][1]
            med = lambda f: statistics.median(f(t, c) for t, c in recs)
            nodes_t = torch.as_tensor(B._clique_bases(bases)[0], device="cuda:0")
            signs_t = torch.as_tensor(B._clique_bases(bases)[1], device="cuda:0").to(torch.float64)
            trecs = timed(lambda: torch_extend(torch, X, nodes_t, signs_t, (q + 1) / 2, gib), min(runs, 2))
            tv = trecs[-1][1][0].cpu().numpy()
            r[q] = dict(n_base=len(nodes_t), wall=med(lambda t, c: t), library=med(lambda t, c: c.seconds),
                        sweep=med(lambda t, c: c.sweep_seconds), rate=med(lambda t, c: c.scanned / c.sweep_seconds),
                        scanned=cuts.scanned, rows=len(cuts), violated=cuts.violated_bases,
                        worst=float(cuts.violations[0]) if len(cuts) else float("nan"),
                        least=float(cuts.violations[-1]) if len(cuts) else float("nan"), allocated=cuts.bytes_allocated,
                        torch_wall=statistics.median(t for t, _ in trecs), torch_worst=float(tv.max()))
            if q == 3:
                five = cuts
            bases = cuts
        if n == max(sizes):                                          # one round: separate, change_rows, warm re-solve
            _, t_sep = clock(lambda: mdl.separate_cliques(first, tri[-1]))
            ch, t_change = clock(lambda: mdl.change_rows(add=five.add))
            sol, t_solve = clock(lambda: mdl.solve(start=ch.carry(first), device_out=True))
            r["round"] = dict(rows=len(five), separate=t_sep, change=t_change, solve=t_solve, iter=int(sol.iter), status=int(sol.status),
                              objval=float(sol.objval), dual_objval=float(sol.dual_objval), first_dual=float(first.dual_objval),
                              left=float(sol.slack_in[-len(five):].max()))
        mdl.close()
        res[n] = r
        print(n, r, flush=True)
    return res


def report(res, runs, nbases, out):
    lines = ["# Pentagonal and heptagonal separation on the device (tools/measure_clique_cuts.py)", "",
             "Max-Cut, G(n, p) with average degree 12, seed 0; reference default options; one MI355X, otherwise idle.  The bases",
             f"of `q = 3` are the {nbases} most violated triangle rows of the first solution of a kept model",
             "(`Model.separate_triangles`), the bases of `q = 5` the pentagonal rows that `q = 3` returned; min_violation 1e-3.",
             "Seconds; `wall`, `library` (proxsdp_clique_cuts.seconds) and `sweep` (sweep_seconds: the sweep kernels alone) are",
             f"medians of {runs} calls after one warm-up call.  `rate` = evaluations scanned / sweep.  `torch` = the same extension",
             "written with whole tensors in torch on the device, batched over bases (first maximum per base, no merge, no rows):",
             "median of 2 calls after one warm-up call.", "",
             "| n | q | bases | wall | library | sweep | evaluations | rate, 1/s | rows | largest violation | smallest | scratch, MiB | torch wall |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in sorted(res):
        for q in (3, 5):
            d = res[n][q]
            lines.append("| %d | %d | %d | %.4f | %.4f | %.4f | %.3e | %.3e | %d | %.4f | %.4f | %.1f | %.4f |" % (
                n, q, d["n_base"], d["wall"], d["library"], d["sweep"], d["scanned"], d["rate"], d["rows"], d["worst"], d["least"],
                d["allocated"] / 2.0 ** 20, d["torch_wall"]))
    lines += ["", "The triangle sweep in the same session (`Model.separate_triangles`, first sweep of the call): " +
              ", ".join("n = %d: %.4f s, %.3e evaluations/s" % (n, res[n]["tri_sweep"], res[n]["tri_rate"]) for n in sorted(res)) + "."]
    for n in sorted(res):
        if "round" in res[n]:
            d = res[n]["round"]
            lines += ["", "One round at n = %d from the first solution: separate (q = 3) %.4f s, `change_rows(add=...)` of the %d "
                      "pentagonal rows %.4f s, warm re-solve %.4f s (%d iterations, status %d); objective in the user's sense "
                      "(maximisation) %.6f before (dual %.6f), %.6f after (dual %.6f); the largest G x - h left on the added rows "
                      "%.2e." % (n, d["separate"], d["rows"], d["change"], d["solve"], d["iter"], d["status"], -res[n]["first_objval"],
                                 -d["first_dual"], -d["objval"], -d["dual_objval"], d["left"])]
    lines += ["", "Reading the figures.  An evaluation is one value v of the contract; the sweep spends 12 fp64 additions, three",
              "maxima and one comparison on the four codes of a pair, all on the vector ALU (X[l, m] is an LDS broadcast, t_m one",
              "conflict-free LDS read, t_l one global load per 64 pairs), with two workgroups of four waves per CU.  Where its rate",
              "equals the triangle sweep's, both run at the rate of their fp64 arithmetic; at n = 1000 a call is launch- and",
              "copy-bound (the sweep is a third of the wall time).  The round is taken from the FIRST solution, like the round of",
              "profiles/triangle_cuts.md, where the triangle rows themselves are still violated: read the objective after it against",
              "the primal-dual gap of the solve before it -- both solves stop at the reference's 1e-4 relative tolerances, so a",
              "difference inside that gap says that these rows did not move the bound at this size, not that they loosened it.",
              "tests/test_clique_cuts.py runs the loop in its proper order (triangle rounds first, then the tight triangles as",
              "bases) at n = 60, where the pentagonal rows lower the bound by 0.25 after the triangles have stopped moving it."]
    lines += ["", "First solves: " + ", ".join("n = %d: %d iterations, %.2f s" % (n, res[n]["first_iter"], res[n]["first_wall"])
                                               for n in sorted(res)) + "."]
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--bases", type=int, default=1000)
    ap.add_argument("--torch-gib", type=float, default=4.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "clique_cuts.md"))
    a = ap.parse_args()
    report(measure(a.sizes, a.runs, a.bases, a.torch_gib), a.runs, a.bases, a.out)


if __name__ == "__main__":
    main()
