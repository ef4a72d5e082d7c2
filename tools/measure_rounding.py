"""What the rounding of a kept model's factors costs and finds: writes profiles/rounding.md.

The instance of profiles/triangle_cuts.md -- Max-Cut on G(n, p), average degree 12, seed 0, reference default options -- at
n = 1000 and n = 4000.  One cold solve on a kept model (factors kept, vectors on the device) gives the first solution; one
round of `--rows` triangle rows (separate, change_rows, warm re-solve) gives the second.  On each, for T = 1024 and
T = 16384 trials, in one session on one otherwise idle GPU:

    device     Model.round(solution, trials=T, seed=0, max_sweeps=50) with the factors as CUDA tensors
    torch      (V sqrt(lambda)) @ randn(r, T), sign, the values through one sparse product with the weights -- no search

    wall       the call as Python sees it (device synchronised), median of `--runs` calls after one warm-up call
    library    proxsdp_rounding.seconds
    search     proxsdp_rounding.search_seconds: the search kernel (value, sweeps, value) between two device events
    cut        the best cut in the user's sense (maximisation), before and after the search; bound = the SDP objective

Recorded, not asserted.

    python tools/measure_rounding.py [--sizes 1000 4000] [--trials 1024 16384] [--runs 5] [--rows 1000] [--out profiles/rounding.md]
"""
import argparse
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent


def measure(sizes, trials, runs, nrows):
    sys.path.insert(0, str(ROOT))
    import numpy as np
    import scipy.sparse as sp
    import torch                                      # (before the library loads: binding.lib)
    from proxsdp_jl_amd import binding as B
    from proxsdp_jl_amd import problems as P
    if B.device_count() <= 0:
        raise SystemExit("needs a HIP device")
    sync = torch.cuda.synchronize
    dev = "cuda:0"

    def clock(call):
        sync()
        t0 = time.perf_counter()
        out = call()
        sync()
        return out, time.perf_counter() - t0

    def torch_rounding(Vd, lam_d, W, dsum, T, gen):
        Y = (Vd * torch.sqrt(lam_d)[None, :]) @ torch.randn(Vd.shape[1], T, device=dev, dtype=torch.float64, generator=gen)
        S = torch.where(Y < 0, -1.0, 1.0).to(torch.float64)
        vals = dsum + 0.5 * (S * torch.sparse.mm(W, S)).sum(dim=0)
        return float(vals.min())

    B.solve(P.maxcut(150, seed=0), B.default_options(), device_out=True)      # (loads the code objects)
    res = {}
    for n in sizes:
        pr = P.maxcut(n, seed=0)
        # the objective as a symmetric weight matrix and a diagonal, for the torch rounding
        jj = np.repeat(np.arange(n), np.arange(1, n + 1))
        ii = np.concatenate([np.arange(j + 1) for j in range(n)])
        off = (ii != jj) & (pr.c != 0.0)
        Wh = sp.coo_matrix((pr.c[off], (ii[off], jj[off])), shape=(n, n))
        Wh = (Wh + Wh.T).tocsr()
        W = torch.sparse_csr_tensor(torch.as_tensor(Wh.indptr, dtype=torch.int64), torch.as_tensor(Wh.indices, dtype=torch.int64),
                                    torch.as_tensor(Wh.data), size=(n, n), device=dev)
        dsum = float(pr.c[ii == jj].sum())
        mdl = B.Model(pr, B.default_options())
        first, t_first = clock(lambda: mdl.solve(factors=True, device_out=True))
        cuts = mdl.separate_triangles(first, count=nrows)
        ch = mdl.change_rows(add=cuts.add)
        second, t_second = clock(lambda: mdl.solve(start=ch.carry(first), factors=True, device_out=True))
        r = dict(first_iter=int(first.iter), first_wall=t_first, second_iter=int(second.iter), second_wall=t_second, rows=len(cuts),
                 points=[])
        for name, sol in (("first", first), (f"after {len(cuts)} rows", second)):
            lam, V = sol.psd_factors[0][:2]
            lam_d, Vd = torch.as_tensor(lam, device=dev), torch.as_tensor(np.ascontiguousarray(V), device=dev)
            for T in trials:
                gen = torch.Generator(device=dev)
                gen.manual_seed(0)
                recs, told = [], []
                for k in range(runs + 1):
                    got, t = clock(lambda: mdl.round((lam_d, Vd), trials=T, seed=0, max_sweeps=50))
                    best_t, t_t = clock(lambda: torch_rounding(Vd, lam_d, W, dsum, T, gen))
                    if k:
                        recs.append(dict(wall=t, library=got.seconds, search=got.search_seconds))
                        told.append(t_t)
                med = lambda key: statistics.median(x[key] for x in recs)
                bound = -float(sol.objval)
                r["points"].append(dict(solution=name, T=T, rank=len(lam), wall=med("wall"), library=med("library"), search=med("search"),
                                        sweeps=got.sweeps, flips=got.flips, cut_rounded=-got.value_rounded, cut=-got.value,
                                        bound=bound, ratio=-got.value / bound, allocated=got.bytes_allocated,
                                        torch_wall=statistics.median(told), torch_cut=-best_t))
        mdl.close()
        res[n] = r
        print(n, r, flush=True)
    return res


def report(res, runs, out):
    lines = ["# Rounding a kept model's factors to a cut on the device, beside a torch rounding (tools/measure_rounding.py)", "",
             "Max-Cut, G(n, p) with average degree 12, seed 0; reference default options; one MI355X, otherwise idle.  `first` =",
             "the first solution of a kept model, the other = the warm re-solve after one round of triangle rows",
             "(`separate_triangles`, `change_rows`).  `device` = `Model.round(factors on the device, trials=T, seed=0,",
             "max_sweeps=50)`: hyperplane rounding and the one-flip search; `torch` = `(V sqrt(lambda)) @ randn`, `sign`, the values",
             "through a sparse product, no search, on the same device in the same session.  Seconds; `wall`, `library`",
             f"(proxsdp_rounding.seconds) and `search` (search_seconds: the search kernel alone) are medians of {runs} calls after",
             "one warm-up call, the two roundings alternating.  Cuts and the bound (the SDP objective) are in the user's sense",
             "(maximisation); `ratio` = cut after the search / bound.  The torch cut is the last call's (its directions differ",
             "from call to call).", "",
             "| n | solution | rank | T | wall | library | search | sweeps | flips | cut rounded | cut | bound | ratio | scratch, MiB | torch wall | torch cut |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in sorted(res):
        for p in res[n]["points"]:
            lines.append("| %d | %s | %d | %d | %.4f | %.4f | %.4f | %d | %d | %.1f | %.1f | %.3f | %.4f | %.1f | %.4f | %.1f |" % (
                n, p["solution"], p["rank"], p["T"], p["wall"], p["library"], p["search"], p["sweeps"], p["flips"], p["cut_rounded"],
                p["cut"], p["bound"], p["ratio"], p["allocated"] / 2.0 ** 20, p["torch_wall"], p["torch_cut"]))
    lines += ["", "Solves: " + ", ".join("n = %d: %d iterations, %.2f s, then %d iterations, %.2f s with %d rows" % (
        n, res[n]["first_iter"], res[n]["first_wall"], res[n]["second_iter"], res[n]["second_wall"], res[n]["rows"]) for n in sorted(res)) + "."]
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4000])
    ap.add_argument("--trials", type=int, nargs="+", default=[1024, 16384])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rounding.md"))
    a = ap.parse_args()
    report(measure(a.sizes, a.trials, a.runs, a.rows), a.runs, a.out)


if __name__ == "__main__":
    main()
