"""What a row change on a kept model costs beside destroy + create: writes profiles/model_rows.md.

The instance of profiles/model_handle.md -- Max-Cut on G(n, p), average degree 12, seed 0, reference default options -- at
n = 1000 and n = 4000.  One cold solve on a kept model (factors kept, vectors on the device) gives the first solution; one
cutting-plane round adds the 1000 most violated triangle inequalities of it and re-solves warm from it.  The separation runs
with torch on the device over the triples {i, j, k} with i in a seeded sample of 64 nodes (all 4 sign patterns, every j < k):
enough to find 1000 violated rows, and the same rows for both routes.  Each figure is the median of `--runs` rounds after one
warm-up round, on one otherwise idle GPU, both routes in the same session:

    rows       Model.change_rows(add=rows) on the kept model, then Model.solve(start=change.carry(first))
    recreate   the route without the row change: Model.close() + Model(changed problem), then Model.solve(start=the same)

    change     wall time of change_rows / of close() + Model(...) as Python sees it (device synchronised)
    library    proxsdp_model_rows.seconds / proxsdp_model_info.setup_time: what the call spends in the library
    allocated  proxsdp_model_rows.bytes_allocated / the new model's device_bytes
    solve      wall time of the warm re-solve; iterations must agree between the routes
    round      change + solve

and, for the share of the support rebuild in a change, the calls alone: dropping those rows again, and adding / dropping as
many rows over diagonal entries (columns that are in the support already, so nothing but the Q- and nnz-sized stages runs).

Recorded, not asserted.

    python tools/measure_model_rows.py [--sizes 1000 4000] [--runs 5] [--rows 1000] [--out profiles/model_rows.md]
"""
import argparse
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
SIGNS = ((-1.0, -1.0, -1.0), (-1.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, 1.0, -1.0))


def separate(torch, primal, side, count, sample=64, seed=0):
    """the `count` most violated triangle rows s . (X_ij, X_ik, X_jk) <= 1 over the triples with i in a seeded sample of nodes;
    returns [(violation, (i, j, k) sorted, sign pattern)] in descending violation, every (triple, pattern) once"""
    dev = primal.device
    lo = torch.tril_indices(side, side, device=dev)              # (row r, col c <= r) in the packed triangle's order
    X = torch.zeros(side, side, dtype=torch.float64, device=dev)
    X[lo[1], lo[0]] = primal
    X[lo[0], lo[1]] = primal
    g = torch.Generator().manual_seed(seed)
    nodes = torch.randperm(side, generator=g)[:min(sample, side)].tolist()
    upper = torch.triu(torch.ones(side, side, dtype=torch.bool, device=dev), diagonal=1)
    found = {}
    for i in nodes:
        a = X[i]
        ok = upper.clone()
        ok[i, :] = False
        ok[:, i] = False
        for s, (s1, s2, s3) in enumerate(SIGNS):
            v = s1 * a[:, None] + s2 * a[None, :] + s3 * X - 1.0
            v = torch.where(ok, v, torch.full_like(v, -1.0))
            top = torch.topk(v.reshape(-1), min(count, v.numel()))
            for val, at in zip(top.values.tolist(), top.indices.tolist()):
                if val <= 0.0:
                    break
                j, k = divmod(at, side)
                # (the pattern is attached to the roles i, j, k: entries X_ij, X_ik, X_jk in that order)
                found[(i, j, k, s)] = val
    best = sorted(found.items(), key=lambda kv: -kv[1])
    out, seen = [], set()
    for (i, j, k, s), val in best:
        # the same inequality reached from another sampled node: its entries as a sorted set of (pair, sign)
        key = frozenset(((min(a, b), max(a, b)), sg) for (a, b), sg in zip(((i, j), (i, k), (j, k)), SIGNS[s]))
        if key in seen:
            continue
        seen.add(key)
        out.append((val, (i, j, k), s))
        if len(out) == count:
            break
    return out


def rows_of(np, P, cuts):
    ptr, cols, vals = [0], [], []
    for _, (i, j, k), s in cuts:
        cols += [int(P.tri_index(i, j)), int(P.tri_index(i, k)), int(P.tri_index(j, k))]
        vals += list(SIGNS[s])
        ptr.append(len(cols))
    return (np.array(ptr, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(vals)), np.ones(len(cuts))


def measure(sizes, runs, nrows):
    sys.path.insert(0, str(ROOT))
    import numpy as np
    import scipy.sparse as sp
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

    B.solve(P.maxcut(150, seed=0), B.default_options(), device_out=True)      # (loads the code objects)
    res = {}
    for n in sizes:
        pr = P.maxcut(n, seed=0)
        mdl = B.Model(pr, B.default_options())
        first = mdl.solve(factors=True, device_out=True)
        cuts = separate(torch, first.primal, n, nrows)
        add = rows_of(np, P, cuts)
        (ptr, cols, vals), h_new = add
        G2 = sp.csr_matrix((vals, cols, ptr), shape=(len(h_new), pr.n)).tocsc()
        pr2 = P.Problem(n=pr.n, A=pr.A, b=pr.b, G=G2, h=h_new, c=pr.c, psd=pr.psd, soc=pr.soc, max_sense=pr.max_sense)
        rec = {"rows": [], "recreate": []}
        other = B.Model(pr, B.default_options())
        for k in range(runs + 1):
            ch, t_change = clock(lambda: mdl.change_rows(add=add))
            start = ch.carry(first)
            sol, t_solve = clock(lambda: mdl.solve(start=start, device_out=True))
            r = dict(change=t_change, library=ch.seconds, allocated=ch.bytes_allocated, solve=t_solve, iter=int(sol.iter),
                     objval=float(sol.objval), rebuilt=ch.support_rebuilt)
            back, t_drop = clock(lambda: mdl.change_rows(drop=np.arange(len(h_new))))   # (back to the first model: not part of the round)
            r.update(drop=t_drop, drop_library=back.seconds, drop_allocated=back.bytes_allocated, drop_rebuilt=back.support_rebuilt)

            def recreate():
                other.close()
                return B.Model(pr2, B.default_options())
            other, t_create = clock(recreate)
            info = other.info()
            sol2, t_solve2 = clock(lambda: other.solve(start=start, device_out=True))
            q = dict(change=t_create, library=info["setup_time"], allocated=info["device_bytes"], solve=t_solve2,
                     iter=int(sol2.iter), objval=float(sol2.objval), rebuilt=0)
            if k:
                rec["rows"].append(r); rec["recreate"].append(q)
        other.close()
        # the calls alone on rows that leave the support set as it is: three diagonal entries a row
        rng = np.random.default_rng(0)
        dcols = np.concatenate([P.tri_index(d, d) for d in (rng.choice(n, size=3, replace=False) for _ in range(len(h_new)))])
        dadd = ((np.arange(0, 3 * len(h_new) + 1, 3, dtype=np.int64), dcols.astype(np.int64), np.ones(3 * len(h_new))),
                np.full(len(h_new), 4.0))
        calls = []
        for k in range(runs + 1):
            ch, t_add = clock(lambda: mdl.change_rows(add=dadd))
            back, t_drop = clock(lambda: mdl.change_rows(drop=np.arange(len(h_new))))
            if k:
                calls.append(dict(add=t_add, add_library=ch.seconds, add_allocated=ch.bytes_allocated, add_rebuilt=ch.support_rebuilt,
                                  drop=t_drop, drop_library=back.seconds, drop_allocated=back.bytes_allocated,
                                  drop_rebuilt=back.support_rebuilt))
        mdl.close()
        res[n] = dict(first_iter=int(first.iter), first_objval=float(first.objval), found=len(cuts),
                      worst=cuts[0][0] if cuts else 0.0, least=cuts[-1][0] if cuts else 0.0)
        for route, recs in rec.items():
            d = {key: statistics.median(x[key] for x in recs) for key in ("change", "library", "allocated", "solve")}
            d["round"] = statistics.median(x["change"] + x["solve"] for x in recs)
            d["iter"] = sorted({x["iter"] for x in recs})
            d["objval"] = recs[-1]["objval"]
            d["rebuilt"] = recs[-1]["rebuilt"]
            res[n][route] = d
        med = lambda recs, key: statistics.median(x[key] for x in recs)
        res[n]["calls"] = [
            ("add the triangle rows", res[n]["rows"]["change"], res[n]["rows"]["library"], res[n]["rows"]["allocated"], res[n]["rows"]["rebuilt"]),
            ("drop them", med(rec["rows"], "drop"), med(rec["rows"], "drop_library"), med(rec["rows"], "drop_allocated"),
             rec["rows"][-1]["drop_rebuilt"]),
            ("add as many rows over diagonal entries", med(calls, "add"), med(calls, "add_library"), med(calls, "add_allocated"),
             calls[-1]["add_rebuilt"]),
            ("drop them", med(calls, "drop"), med(calls, "drop_library"), med(calls, "drop_allocated"), calls[-1]["drop_rebuilt"])]
        print(n, res[n], flush=True)
    return res


def report(res, runs, nrows, out):
    lines = ["# One cutting-plane round on a kept model: change_rows beside close() + Model(...) (tools/measure_model_rows.py)", "",
             "Max-Cut, G(n, p) with average degree 12, seed 0; reference default options; one MI355X, otherwise idle.  The round adds",
             f"the {nrows} most violated triangle rows of the first solution (separated with torch on the device over the triples",
             "that contain one of 64 seeded nodes) and re-solves warm from that solution, device tensors in and out.  Seconds, the",
             f"median of {runs} rounds after one warm-up round, both routes in one session.  `rows` = `Model.change_rows(add=...)`",
             "on the kept model; `recreate` = `Model.close()` + `Model(changed problem)`, the route without the row change.",
             "`change`: the call's wall time from Python; `library`: proxsdp_model_rows.seconds / proxsdp_model_info.setup_time;",
             "`allocated`: proxsdp_model_rows.bytes_allocated / the new model's device_bytes; `solve`: the warm re-solve's wall",
             "time; `round` = change + solve.", "",
             "| n | route | rows added | change | library | allocated, MiB | solve | iterations | round |",
             "|---|---|---|---|---|---|---|---|---|"]
    for n in sorted(res):
        for route in ("rows", "recreate"):
            d = res[n][route]
            lines.append("| %d | %s | %d | %.4f | %.4f | %.1f | %.4f | %s | %.4f |" % (
                n, route, res[n]["found"], d["change"], d["library"], d["allocated"] / 2.0 ** 20, d["solve"],
                ", ".join(str(v) for v in d["iter"]), d["round"]))
    lines += ["", "| n | first solve, iterations | largest violation | smallest added | objective before | after (rows) | after (recreate) | "
              "support rebuilt | change, rows / recreate | round, rows / recreate |", "|---|---|---|---|---|---|---|---|---|---|"]
    for n in sorted(res):
        a, b = res[n]["rows"], res[n]["recreate"]
        lines.append("| %d | %d | %.4f | %.4f | %.6f | %.6f | %.6f | %d | %.3f | %.3f |" % (
            n, res[n]["first_iter"], res[n]["worst"], res[n]["least"], -res[n]["first_objval"], -a["objval"], -b["objval"],
            a["rebuilt"], a["change"] / b["change"], a["round"] / b["round"]))
    lines += ["", "The calls alone (`rows` route; the last column: did the call rebuild the support set):", "",
              "| n | call | wall | library | allocated, MiB | support rebuilt |", "|---|---|---|---|---|---|"]
    for n in sorted(res):
        for label, wall, lib, alloc, rebuilt in res[n]["calls"]:
            lines.append("| %d | %s | %.4f | %.4f | %.1f | %d |" % (n, label, wall, lib, alloc / 2.0 ** 20, rebuilt))
    lines += ["", "The objectives are in the user's sense (maximisation).  A row change redoes the stages of the set-up that read Q, nnz",
              "or the pattern -- the planner on the host, the operator's arrays in both orientations, the Q-sized vectors, the exit",
              "path's arrays and, here, the support set with its ELL structures (the triangle rows bring off-diagonal columns into",
              "it) -- and keeps the Lanczos workspaces, the sign projection's work matrices, x and M'y, streams and rocBLAS."]
    pathlib.Path(out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "model_rows.md"))
    a = ap.parse_args()
    report(measure(a.sizes, a.runs, a.rows), a.runs, a.rows, a.out)


if __name__ == "__main__":
    main()
