"""What the triangle separation on the device costs and finds: writes profiles/triangle_cuts.md.

The instance of profiles/model_rows.md -- Max-Cut on G(n, p), average degree 12, seed 0, reference default options -- at
n = 1000 and n = 4000.  One cold solve on a kept model (factors kept, vectors on the device) gives the first solution.  On that
solution, in one session on one otherwise idle GPU:

    full       Model.separate_triangles(first, count=1000): every one of the 4 C(n, 3) triangle inequalities
    sampled    tools/measure_model_rows.py's torch separation over the triples that contain one of 64 seeded nodes

    wall       the call as Python sees it (device synchronised), median of `--runs` calls after one warm-up call
    library    proxsdp_triangle_cuts.seconds
    sweep      proxsdp_triangle_cuts.sweep_seconds: the first sweep over the triples alone, between two device events
    passes     sweeps of the call (histogram passes of the radix select + the emit pass)

and one full round per separation -- separate, Model.change_rows(add=...), Model.solve(start=change.carry(first)) -- with the
objective before and after it; the rows are dropped again between the two rounds, so both start from the same model.

Recorded, not asserted.

    python tools/measure_triangle_cuts.py [--sizes 1000 4000] [--runs 5] [--rows 1000] [--out profiles/triangle_cuts.md]
"""
import argparse
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent


def measure(sizes, runs, nrows):
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tools"))
    import numpy as np
    import torch                                      # (before the library loads: binding.lib)
    import measure_model_rows as MR
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

    B.solve(P.maxcut(150, seed=0), B.default_options(), device_out=True)      # (loads the code objects)
    res = {}
    for n in sizes:
        pr = P.maxcut(n, seed=0)
        mdl = B.Model(pr, B.default_options())
        first, t_first = clock(lambda: mdl.solve(factors=True, device_out=True))
        full, sampled = [], []
        for k in range(runs + 1):
            cuts, t = clock(lambda: mdl.separate_triangles(first, count=nrows))
            old, t_old = clock(lambda: MR.separate(torch, first.primal, n, nrows))
            if k:
                full.append(dict(wall=t, library=cuts.seconds, sweep=cuts.sweep_seconds))
                sampled.append(dict(wall=t_old))
        med = lambda recs, key: statistics.median(x[key] for x in recs)
        r = dict(first_iter=int(first.iter), first_objval=float(first.objval), first_wall=t_first,
                 full=dict(wall=med(full, "wall"), library=med(full, "library"), sweep=med(full, "sweep"), passes=cuts.passes,
                           violated=cuts.violated, scanned=cuts.scanned, found=len(cuts), worst=float(cuts.violations[0]),
                           least=float(cuts.violations[-1]), allocated=cuts.bytes_allocated),
                 sampled=dict(wall=med(sampled, "wall"), found=len(old), worst=old[0][0], least=old[-1][0]))
        # one round per separation, from the same model and the same start
        for name, add in (("full", cuts.add), ("sampled", MR.rows_of(np, P, old))):
            ch, t_change = clock(lambda: mdl.change_rows(add=add))
            sol, t_solve = clock(lambda: mdl.solve(start=ch.carry(first), device_out=True))
            slack = mdl.inactive_rows(sol)
            r[name].update(change=t_change, solve=t_solve, iter=int(sol.iter), objval=float(sol.objval), status=int(sol.status),
                           round=r[name]["wall"] + t_change + t_solve, inactive=len(slack))
            mdl.change_rows(drop=np.arange(len(add[1])))
        mdl.close()
        res[n] = r
        print(n, r, flush=True)
    return res


def report(res, runs, nrows, out):
    lines = ["# Triangle separation on the device beside the sampled torch separation (tools/measure_triangle_cuts.py)", "",
             "Max-Cut, G(n, p) with average degree 12, seed 0; reference default options; one MI355X, otherwise idle.  Both",
             f"separations read the first solution of a kept model on the device and return {nrows} rows.  `full` =",
             "`Model.separate_triangles` (all 4 C(n, 3) inequalities, min_violation 1e-3); `sampled` = the torch separation of",
             "tools/measure_model_rows.py (the triples that contain one of 64 seeded nodes).  Seconds; `wall`, `library`",
             f"(proxsdp_triangle_cuts.seconds) and `sweep` (sweep_seconds: one sweep over the triples) are medians of {runs} calls",
             "after one warm-up call, both separations alternating in one session.", "",
             "| n | separation | wall | library | sweep | passes | rows scanned | violated | largest violation | smallest returned | scratch, MiB |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in sorted(res):
        f, s = res[n]["full"], res[n]["sampled"]
        lines.append("| %d | full | %.4f | %.4f | %.4f | %d | %.3e | %d | %.4f | %.4f | %.1f |" % (
            n, f["wall"], f["library"], f["sweep"], f["passes"], f["scanned"], f["violated"], f["worst"], f["least"],
            f["allocated"] / 2.0 ** 20))
        lines.append("| %d | sampled | %.4f | | | | | | %.4f | %.4f | |" % (n, s["wall"], s["worst"], s["least"]))
    lines += ["", "One round from the first solution: separate, `change_rows(add=...)`, warm re-solve (`round` = the three together;",
              "`slack rows` = `Model.inactive_rows` of the second solution, default tolerances).  The objectives are in the user's",
              "sense (maximisation).  `change_rows` and the re-solve are single runs, the full round first; the rows of the full",
              "separation are spread over all nodes, so they bring more columns into the support set than the sampled ones.", "",
              "| n | separation | separate | change_rows | re-solve | iterations | status | round | objective before | after | slack rows |",
              "|---|---|---|---|---|---|---|---|---|---|---|"]
    for n in sorted(res):
        for name in ("full", "sampled"):
            d = res[n][name]
            lines.append("| %d | %s | %.4f | %.4f | %.4f | %d | %d | %.4f | %.6f | %.6f | %d |" % (
                n, name, d["wall"], d["change"], d["solve"], d["iter"], d["status"], d["round"], -res[n]["first_objval"],
                -d["objval"], d["inactive"]))
    lines += ["", "First solves: " + ", ".join("n = %d: %d iterations, %.2f s" % (n, res[n]["first_iter"], res[n]["first_wall"])
                                               for n in sorted(res)) + "."]
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "triangle_cuts.md"))
    a = ap.parse_args()
    report(measure(a.sizes, a.runs, a.rows), a.runs, a.rows, a.out)


if __name__ == "__main__":
    main()
