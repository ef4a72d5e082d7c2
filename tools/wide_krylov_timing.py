"""Wide Lanczos (options.lanczos_wide_krylov = 1) against the narrow step kernels and the dense stand-in.

1. One eigsolve per (n, K) on a random packed matrix (Wigner spectrum: a Krylov dimension's worth of steps per cycle),
   bounded to --eig-cycles cycles (krylovkit_max_iter): wall time per Lanczos step, the restart rotations included;
   the narrow step kernels at K = 255, the wide kernels above.
2. PDHG iterations/s on Max-Cut at target rank 128 and 181 (Krylov dimension 257 / 363) with the option at 0 (dense
   stand-in) and 1 (wide kernels): ONE solve per setting, --settle untimed iterations, then a window of --iters
   iterations timed from the solver's own trace (column 12, seconds since the start), as bench.py does.  The target
   rank is pinned by initial_target_rank; max_target_rank_krylov_eigs = rank + 64 keeps the Krylov branch when the
   rank schedule moves it up.  Reported with the window's projections by engine.
Prints one JSON line per measurement.  Usage: python tools/wide_krylov_timing.py [--sizes 4000 16384] [--iters 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from proxsdp_jl_amd import binding as B          # noqa: E402
from proxsdp_jl_amd import problems as P         # noqa: E402
from proxsdp_jl_amd.optimizer import Optimizer   # noqa: E402


def eig_timing(n, K, cycles):
    nev = (K - 1) // 2
    x = np.random.default_rng(n).standard_normal(n * (n + 1) // 2)
    o = B.default_options()
    B.set_option(o, "lanczos_wide_krylov", 1)
    B.set_option(o, "krylovkit_max_iter", cycles)
    B.eigsolve(x, n, nev, options=o, cap=K + 1)               # warm-up (allocation, code objects)
    t0 = time.perf_counter()
    _, _, info = B.eigsolve(x, n, nev, options=o, cap=K + 1)
    dt = time.perf_counter() - t0
    return dict(kind="eigsolve", n=n, K=K, wide=K > 255, s=dt, nmatvec=info["nmatvec"], numiter=info["numiter"],
                us_per_step=1e6 * dt / max(info["nmatvec"], 1))


def pdhg_timing(pr, n, rank, wide, settle, iters):
    tot = settle + iters
    kw = dict(max_target_rank_krylov_eigs=rank + 64, initial_target_rank=rank, lanczos_wide_krylov=int(wide),
              max_iter=tot, min_iter=tot)
    t0 = time.perf_counter()
    sol = Optimizer(**kw).optimize(pr, trace_capacity=tot)
    wall = time.perf_counter() - t0
    tr = sol.trace
    if len(tr) < tot:
        return dict(kind="pdhg", n=n, rank=rank, wide=wide, error=f"stopped after {len(tr)} iterations")
    t = float(tr[tot - 1, 12] - tr[settle - 1, 12])
    return dict(kind="pdhg", n=n, rank=rank, wide=wide, settle=settle, iters=iters, window_s=t, it_per_s=iters / t,
                target_rank_window=sorted(set(int(r) for r in tr[settle:tot, 10])),
                matvecs_per_it=float(tr[settle:tot, 13].mean()), solve_wall_s=wall,
                wide_projections=sol.stats["wide_krylov_projections"], dense=sol.stats["dense_truncated_projections"],
                full_eigs=sol.stats["full_eigs"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[4000])
    ap.add_argument("--eig-K", type=int, nargs="+", default=[255, 321, 401, 511])
    ap.add_argument("--eig-cycles", type=int, default=2)
    ap.add_argument("--ranks", type=int, nargs="+", default=[128, 181])
    ap.add_argument("--settle", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--skip-eig", action="store_true")
    ap.add_argument("--skip-pdhg", action="store_true")
    a = ap.parse_args()
    for n in a.sizes:
        if not a.skip_eig:
            for K in a.eig_K:
                print(json.dumps(eig_timing(n, K, a.eig_cycles)), flush=True)
        if not a.skip_pdhg:
            pr = P.maxcut(n, seed=0)
            for rank in a.ranks:
                for wide in (False, True):
                    print(json.dumps(pdhg_timing(pr, n, rank, wide, a.settle, a.iters)), flush=True)
