"""Per-iteration time (trace column 12 / iterations) of the SECOND solve of a process: single process, in-process 2 shards,
2 gloo ranks; on the coupled two-Max-Cut model and MIMO 8 x 513 split 4 + 4.  Driver without arguments: every leg in a fresh
child with its own time limit, stops at the first failure; one RESULT line of JSON per leg (profiles/inprocess_shards.md)."""
import json
import multiprocessing as mp
import os
import pathlib
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def model(name):
    import numpy as np
    import scipy.sparse as sp
    from proxsdp_jl_amd import problems as P
    if name == "mimo":
        return P.block_diag_problems([P.mimo(512, seed=s_) for s_ in range(8)], name="mimo-x8"), 400
    pr = P.block_diag_problems([P.maxcut(120, seed=1), P.maxcut(150, seed=2)], name="two-maxcut")
    n1 = P.maxcut(120, seed=1).n
    row = sp.csr_matrix(([1.0, 2.0], ([0, 0], [0, n1])), shape=(1, pr.n))
    g = sp.csr_matrix(([1.0, -1.0], ([0, 0], [2, n1 + 2])), shape=(1, pr.n))
    return P.Problem(n=pr.n, A=sp.vstack([pr.A, row]).tocsc(), b=np.append(pr.b, 3.0),
                     G=sp.vstack([pr.G, g]).tocsc(), h=np.append(pr.h, 0.5), c=pr.c, psd=pr.psd, name="two-maxcut-coupled"), 300


def record(sol, stats=None):
    st = stats or sol.stats
    return dict(iter=int(sol.iter), status=int(sol.status), seconds=float(sol.trace[sol.iter - 1, 12]),
                us_per_iter=1e6 * float(sol.trace[sol.iter - 1, 12]) / int(sol.iter),
                matvecs=int(st["lanczos_matvecs"]), restarts=int(st["lanczos_restarts"]), objval=float(sol.objval))


def _gloo_worker(rank, world, port, q, name):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from proxsdp_jl_amd import replicas, sharded
    dist = replicas.init("gloo", rank, world)
    pr, mi = model(name)
    recs = []
    for _ in range(2):
        opt, sol, maps = sharded.solve_sharded(pr, dist, rank, world, device_id=0, max_iter=mi)
        recs.append(record(sol))
    q.put((rank, recs))
    dist.destroy_process_group()


def leg(kind, name):
    from proxsdp_jl_amd.optimizer import Optimizer
    pr, mi = model(name)
    if kind == "gloo":
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        procs = [ctx.Process(target=_gloo_worker, args=(r, 2, 29871, q, name)) for r in range(2)]
        for p in procs:
            p.start()
        try:
            out = sorted((q.get(timeout=500) for _ in procs), key=lambda t: t[0])
            for p in procs:
                p.join(timeout=60)
        finally:
            for p in procs:
                if p.is_alive():
                    p.kill()
        recs = []
        for k in range(2):
            r0, r1 = out[0][1][k], out[1][1][k]
            assert r0["iter"] == r1["iter"]
            recs.append(dict(r0, us_per_iter=max(r0["us_per_iter"], r1["us_per_iter"]), seconds=max(r0["seconds"], r1["seconds"]),
                             matvecs=r0["matvecs"] + r1["matvecs"], restarts=r0["restarts"] + r1["restarts"],
                             us_per_iter_ranks=[r0["us_per_iter"], r1["us_per_iter"]]))
    else:
        recs = []
        for _ in range(2):
            if kind == "single":
                sol = Optimizer(max_iter=mi, support_path=1).optimize(pr, trace_capacity=mi)
                recs.append(record(sol))
            else:
                opt = Optimizer(max_iter=mi)
                sol = opt.optimize(pr, trace_capacity=mi, shards=2, device_ids=[0, 0])
                r = record(sol)
                r["general_iterations"] = [int(s["sharded_general_iterations"]) for s in opt.shard_stats]
                r["batched_block_steps"] = [int(s["batched_block_steps"]) for s in opt.shard_stats]
                recs.append(r)
    print("RESULT " + json.dumps(dict(model=name, leg=kind, first=recs[0], second=recs[1])), flush=True)


def driver():
    results = []
    for name in ("maxcut", "mimo"):
        for kind in ("single", "inproc", "gloo"):
            import signal
            from types import SimpleNamespace
            pp = subprocess.Popen([sys.executable, __file__, kind, name], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                  text=True, start_new_session=True)
            try:
                so, _ = pp.communicate(timeout=240 if name == "mimo" else 120)
                r = SimpleNamespace(stdout=so, returncode=pp.returncode)
            except subprocess.TimeoutExpired:
                os.killpg(pp.pid, signal.SIGKILL)
                so, _ = pp.communicate()
                print("TIMEOUT", name, kind, (so or "")[-2000:], flush=True)
                return 124
            if r.returncode != 0:
                print("FAILED", name, kind, r.returncode, r.stdout[-3000:], flush=True)
                return 1
            for line in r.stdout.splitlines():
                if line.startswith("RESULT "):
                    results.append(json.loads(line[7:]))
                    print(line, flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3:
        leg(sys.argv[1], sys.argv[2])
    else:
        sys.exit(driver())
