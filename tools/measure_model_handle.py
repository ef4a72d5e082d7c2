"""What a model handle saves on a warm re-solve: writes profiles/model_handle.md.

The instance of profiles/device_results.md -- Max-Cut on G(n, p), average degree 12, seed 0, reference default options -- at
n = 1000 and n = 4000.  One cold solve (factors kept, vectors on the device) gives the start point; then, each the median of
`--runs` runs after one warm-up run, on one otherwise idle GPU:

    parent        solve(start=prev_device, device_out=True) with the library of the parent commit (--parent DIR: a checkout
                  of it with its library built; measured in a child process of its own; left out when not given)
    call          the same call with this commit's library (proxsdp_hip_solve_device: everything set up per call)
    model         Model.solve(start=prev_device, device_out=True) on a handle created before the clock starts
    model, 1 %    Model.update(c=...) with every edge weight changed by a seeded +-1 %, then the same Model.solve; `update`
                  is the update's own wall time (host route: a NumPy array), the other columns are the solve's

    wall          the whole call as Python sees it (device synchronised before the clock stops)
    init, loop    stats.init_time, stats.loop_time
    exit          stats.exit_time
    marshalling   wall - init - loop - exit

and once per size: `create` = proxsdp_model_info.setup_time, what Model(...) spends in the library.  Recorded, not asserted.

    python tools/measure_model_handle.py [--sizes 1000 4000] [--runs 5] [--parent DIR] [--out profiles/model_handle.md]
"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
PARTS = ("wall", "init", "loop", "exit", "marshalling")


def measure(root, route, sizes, runs):
    """{n: {row: {part: median seconds, "iter": iterations, ...}}} with the package under `root`"""
    sys.path.insert(0, str(root))
    import numpy as np
    import torch                                      # (before the library loads: binding.lib)
    from proxsdp_jl_amd import binding as B
    from proxsdp_jl_amd import problems as P
    if B.device_count() <= 0:
        raise SystemExit("needs a HIP device")
    sync = torch.cuda.synchronize

    def timed(call):
        sync()
        t0 = time.perf_counter()
        sol = call()
        sync()
        wall = time.perf_counter() - t0
        st = sol.stats
        rec = dict(wall=wall, init=st["init_time"], loop=st["loop_time"], exit=st["exit_time"])
        rec["marshalling"] = wall - rec["init"] - rec["loop"] - rec["exit"]
        return sol, rec

    def median(recs, sol, **more):
        out = {k: statistics.median(r[k] for r in recs) for k in PARTS}
        out["iter"] = int(sol.iter)
        out.update(more)
        return out

    def repeat(call):
        sol, recs = None, []
        for k in range(runs + 1):
            sol, rec = timed(call)
            if k:
                recs.append(rec)
        return sol, recs

    B.solve(P.maxcut(150, seed=0), B.default_options(), device_out=True)      # (loads the code objects)
    res = {}
    for n in sizes:
        pr = P.maxcut(n, seed=0)
        cold = B.solve(pr, B.default_options(), factors=True, device_out=True)
        res[n] = {}
        if route != "model":
            sol, recs = repeat(lambda: B.solve(pr, B.default_options(), start=cold, device_out=True))
            res[n]["warm"] = median(recs, sol)
        else:
            rng = np.random.default_rng(0)
            c2 = pr.c * (1.0 + 0.01 * rng.choice([-1.0, 1.0], size=len(pr.c)))
            with B.Model(pr, B.default_options()) as mdl:
                create = mdl.info()["setup_time"]
                sol, recs = repeat(lambda: mdl.solve(start=cold, device_out=True))
                res[n]["warm"] = median(recs, sol, create=create)
                ups, recs, sol = [], [], None
                for k in range(runs + 1):
                    sync()
                    t0 = time.perf_counter()
                    mdl.update(c=c2 if k % 2 == 0 else pr.c * (2.0 - c2 / np.where(pr.c != 0.0, pr.c, 1.0)))
                    up = time.perf_counter() - t0
                    sol, rec = timed(lambda: mdl.solve(start=cold, device_out=True))
                    if k:
                        ups.append(up); recs.append(rec)
                res[n]["perturbed"] = median(recs, sol, update=statistics.median(ups),
                                             rebuilds=int(mdl.info()["support_rebuilds"]))
        print(route, n, json.dumps(res[n]), flush=True)
    return res


def report(results, runs, out):
    lines = ["# A model kept on the device: the warm re-solve without its set-up (tools/measure_model_handle.py)", "",
             "Max-Cut, G(n, p) with average degree 12, seed 0; reference default options; one MI355X, otherwise idle.  Seconds,",
             f"the median of {runs} runs after one warm-up run.  `wall`: the whole call seen from Python; `init`, `loop`, `exit`:",
             "stats.init_time, stats.loop_time, stats.exit_time; `marshalling` = wall - init - loop - exit.  Every row is the warm",
             "re-solve from a cold solve's factors and duals, device tensors in and out.  Routes: `parent` =",
             "`solve(start=prev_device, device_out=True)` with the parent commit's library, `call` = the same call with this commit's",
             "library, `model` = `Model.solve(start=prev_device, device_out=True)` on a handle that exists already, `model, 1 %` = the",
             "same after `Model.update(c=...)` with every edge weight changed by a seeded +-1 % (`update`: that call's own wall time,",
             "host route).", "",
             "| n | route | iterations | wall | init | loop | exit | marshalling | update |", "|---|---|---|---|---|---|---|---|---|"]
    routes = [r for r in ("parent", "call", "model") if r in results]
    sizes = sorted({int(n) for r in routes for n in results[r]})
    rows = {}
    for n in sizes:
        for r in routes:
            for run, label in (("warm", r), ("perturbed", r + ", 1 %")):
                d = results[r][str(n)].get(run)
                if d is None:
                    continue
                rows[(n, label)] = d
                lines.append("| %d | %s | %d | %s | %s |" % (n, label, d["iter"], " | ".join("%.4f" % d[k] for k in PARTS),
                                                             "%.4f" % d["update"] if "update" in d else ""))
    base = "parent" if "parent" in results else "call"
    lines += ["", f"## Against the {base} route", "", "| n | route | wall, ratio | wall - loop, ratio | create, seconds |",
              "|---|---|---|---|---|"]
    for n in sizes:
        b = rows[(n, base)]
        for (nn, label), d in rows.items():
            if nn != n or label == base:
                continue
            lines.append("| %d | %s | %.3f | %.3f | %s |" % (n, label, d["wall"] / b["wall"],
                                                             (d["wall"] - d["loop"]) / (b["wall"] - b["loop"]),
                                                             "%.4f" % d["create"] if "create" in d else ""))
    lines += ["", "`create` is proxsdp_model_info.setup_time: validation, ordering, scaling, the operator in both orientations, the",
              "workspaces and the exit path's arrays, paid once per handle instead of once per solve.  A handle's `init` is the reset",
              "of what the last solve wrote and the start path; its `marshalling` is the result tensors and the start's ctypes structs.",
              "`wall - loop` is everything a re-solve pays around its iterations."]
    pathlib.Path(out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "model_handle.md"))
    ap.add_argument("--child", nargs=3, metavar=("ROOT", "ROUTE", "JSON"), help="(internal) measure one route into a JSON file")
    a = ap.parse_args()
    if a.child:
        pathlib.Path(a.child[2]).write_text(json.dumps(measure(pathlib.Path(a.child[0]), a.child[1], a.sizes, a.runs)))
        return
    results = {}
    todo = ([("parent", a.parent, "call")] if a.parent else []) + [("call", str(ROOT), "call"), ("model", str(ROOT), "model")]
    with tempfile.TemporaryDirectory() as tmp:
        for name, root, route in todo:                # one fresh process per route: its own runtime, allocator and caches
            js = str(pathlib.Path(tmp) / (name + ".json"))
            subprocess.run([sys.executable, __file__, "--child", root, route, js, "--runs", str(a.runs), "--sizes"] +
                           [str(n) for n in a.sizes], check=True)
            results[name] = json.loads(pathlib.Path(js).read_text())
    report(results, a.runs, a.out)


if __name__ == "__main__":
    main()
