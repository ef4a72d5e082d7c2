"""Where a solve's wall time goes outside the loop, host exit path against device exit path: writes profiles/device_results.md.

The instance of profiles/warm_start.md -- Max-Cut on G(n, p), average degree 12, seed 0, reference default options -- at
n = 1000 and n = 4000.  For the cold solve (factors kept) and for the warm re-solve from its own factors and duals:

    wall          the whole call as Python sees it (device synchronised before the clock stops)
    init, loop    stats.init_time, stats.loop_time
    exit          stats.exit_time (cache_solution, or cache_solution_device)
    marshalling   wall - init - loop - exit: ctypes marshalling, preprocessing, result arrays

through three routes, each the median of `--runs` runs after one warm-up run, on one otherwise idle GPU:

    parent        solve(start=prev) with the library of the parent commit (--parent DIR: a checkout of it with its library
                  built; measured in a child process of its own; left out when not given)
    host          the same call with this commit's library (proxsdp_hip_solve_factored / _solve_from: the host exit path)
    device        solve(start=prev_device, device_out=True) (proxsdp_hip_solve_device: the device exit path, tensors in and out)

Recorded, not asserted.

    python tools/measure_device_results.py [--sizes 1000 4000] [--runs 5] [--parent DIR] [--out profiles/device_results.md]
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
    """{n: {"cold" | "warm": {part: median seconds, "iter": iterations}}} with the package under `root`"""
    sys.path.insert(0, str(root))
    if route == "device":
        import torch                                  # (before the library loads: binding.lib)
    from proxsdp_jl_amd import binding as B
    from proxsdp_jl_amd import problems as P
    if B.device_count() <= 0:
        raise SystemExit("needs a HIP device")
    dev = route == "device"
    kw = dict(device_out=True) if dev else {}
    sync = (lambda: None)
    if dev:
        sync = torch.cuda.synchronize

    def timed(pr, **k):
        sync()
        t0 = time.perf_counter()
        sol = B.solve(pr, B.default_options(), **k, **kw)
        sync()
        wall = time.perf_counter() - t0
        st = sol.stats
        rec = dict(wall=wall, init=st["init_time"], loop=st["loop_time"], exit=st["exit_time"])
        rec["marshalling"] = wall - rec["init"] - rec["loop"] - rec["exit"]
        return sol, rec

    def median(recs, sol):
        out = {k: statistics.median(r[k] for r in recs) for k in PARTS}
        out["iter"] = int(sol.iter)
        return out

    timed(P.maxcut(150, seed=0))                      # (loads the code objects)
    res = {}
    for n in sizes:
        pr = P.maxcut(n, seed=0)
        cold, recs = None, []
        for k in range(runs + 1):
            cold, rec = timed(pr, factors=True)
            if k:
                recs.append(rec)
        res[n] = dict(cold=median(recs, cold))
        warm, recs = None, []
        for k in range(runs + 1):
            warm, rec = timed(pr, start=cold)
            if k:
                recs.append(rec)
        res[n]["warm"] = median(recs, warm)
        print(route, n, json.dumps(res[n]), flush=True)
    return res


def report(results, runs, out):
    lines = ["# Solution vectors on the device: where the time outside the loop goes (tools/measure_device_results.py)", "",
             "Max-Cut, G(n, p) with average degree 12, seed 0; reference default options; one MI355X, otherwise idle.  Seconds,",
             f"the median of {runs} runs after one warm-up run.  `wall`: the whole call seen from Python; `init`, `loop`, `exit`:",
             "stats.init_time, stats.loop_time, stats.exit_time; `marshalling` = wall - init - loop - exit.  Routes: `parent` =",
             "`solve(start=prev)` with the parent commit's library, `host` = the same call with this commit's library (host exit",
             "path), `device` = `solve(start=prev_device, device_out=True)` (proxsdp_hip_solve_device: device exit path, tensors in",
             "and out).  `cold` is `solve(factors=True)`, `warm` the re-solve from that result's factors and duals.", "",
             "| n | run | route | iterations | wall | init | loop | exit | marshalling |", "|---|---|---|---|---|---|---|---|---|"]
    routes = [r for r in ("parent", "host", "device") if r in results]
    sizes = sorted({int(n) for r in routes for n in results[r]})
    for n in sizes:
        for run in ("cold", "warm"):
            for r in routes:
                d = results[r][str(n)][run]
                lines.append("| %d | %s | %s | %d | %s |" % (n, run, r, d["iter"], " | ".join("%.4f" % d[k] for k in PARTS)))
    base = "parent" if "parent" in results else "host"
    lines += ["", f"## Against the {base} route", "", "| n | run | route | exit, ratio | wall, ratio |", "|---|---|---|---|---|"]
    for n in sizes:
        for run in ("cold", "warm"):
            b = results[base][str(n)][run]
            for r in routes:
                if r == base:
                    continue
                d = results[r][str(n)][run]
                lines.append("| %d | %s | %s | %.3f | %.3f |" % (n, run, r, d["exit"] / b["exit"], d["wall"] / b["wall"]))
    lines += ["", "`marshalling` lies outside the library's timers: building the ctypes problem, `prepare()` (the host preprocessing of the",
              "model: it runs before `init_time`'s clock starts) and allocating the result arrays.  Both exit paths pay it alike; a",
              "persistent model handle would remove it."]
    pathlib.Path(out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4000])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "device_results.md"))
    ap.add_argument("--child", nargs=3, metavar=("ROOT", "ROUTE", "JSON"), help="(internal) measure one route into a JSON file")
    a = ap.parse_args()
    if a.child:
        pathlib.Path(a.child[2]).write_text(json.dumps(measure(pathlib.Path(a.child[0]), a.child[1], a.sizes, a.runs)))
        return
    results = {}
    todo = ([("parent", a.parent, "host")] if a.parent else []) + [("host", str(ROOT), "host"), ("device", str(ROOT), "device")]
    with tempfile.TemporaryDirectory() as tmp:
        for name, root, route in todo:                # one fresh process per route: its own runtime, allocator and caches
            js = str(pathlib.Path(tmp) / (name + ".json"))
            subprocess.run([sys.executable, __file__, "--child", root, route, js, "--runs", str(a.runs), "--sizes"] +
                           [str(n) for n in a.sizes], check=True)
            results[name] = json.loads(pathlib.Path(js).read_text())
    report(results, a.runs, a.out)


if __name__ == "__main__":
    main()
