#!/usr/bin/env python
"""Measurements behind profiles/solution_factors.md (needs an MI355X):

    python tools/measure_solution_factors.py [--out profiles/solution_factors.md] [--n 4000] [--iters 300] [--cap 128]

1. Max-Cut n = 120, default options: ||V'V - I||_2 of the returned Ritz vectors beside the CPU oracle's Ritz vectors of the
   same block; the EIG sources (full_eig_decomp = 1, the 3 x 3 KAT, equilibration_force = 1): reported residual over
   numpy's own ||Xk - (Xk)+||_F (LAPACK on the same matrix).
2. The bench instance (Max-Cut n = 4000 pinned at target rank 63, the options of bench.py's headline solve): exit_time of
   the factored solve against the plain solve -- same build, same process, alternating, median of five -- and which cones
   came back RITZ / EIG.
3. k_factor_residual's event time beside k_reconstruct_mfma<false>'s at the same n and r, on that solve's own factors."""
import argparse
import pathlib
import statistics
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import oracle                                            # noqa: E402
from oracle import eig as oeig                           # noqa: E402
from proxsdp_jl_amd import binding as B                  # noqa: E402
from proxsdp_jl_amd import problems as P                 # noqa: E402

U = 2.0 ** -53


def options(**kw):
    o = B.default_options()
    for k, v in kw.items():
        B.set_option(o, k, v)
    return o


def block(x, pr, k):
    return P.unpack_psd(x[pr.psd[k]], B.psd_sides(pr)[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "solution_factors.md"))
    ap.add_argument("--n", type=int, default=4000)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--cap", type=int, default=128)
    ap.add_argument("--repeat", type=int, default=20)
    args = ap.parse_args()
    L = []
    say = lambda s="": (L.append(s), print(s, flush=True))
    say("# Factors of the PSD solution: measurements")
    say()
    say("Made by `tools/measure_solution_factors.py` on an MI355X (one process, one build).")
    say()

    # ---- 1. accuracy figures at n = 120
    pr = P.maxcut(120, seed=0)
    sol = B.solve(pr, options(), factors=True)
    vals, vecs, info = sol.psd_factors[0]
    Xk = block(sol.primal, pr, 0)
    r = info["rank"]
    lib = float(np.linalg.norm(vecs.T @ vecs - np.eye(r), 2))
    o = oracle.Options()
    arc = oeig.EigSolverAlloc(120, o)
    oeig.krylovkit_eig(arc, np.asfortranarray(Xk), r, o)
    k = min(r, arc.converged_eigs)
    Z = np.asarray(arc.vecs)[:, :k]
    ref = float(np.linalg.norm(Z.T @ Z - np.eye(k), 2))
    say("## Max-Cut n = 120, default options")
    say()
    say(f"- status {sol.status}, {sol.iter} iterations, final_rank {sol.final_rank}; source {info['source_name']}, rank {r}")
    say(f"- `||V'V - I||_2`: library {lib:.3e}, CPU oracle's Ritz vectors of the same block {ref:.3e} ({k} pairs), n u = {120 * U:.3e}")
    say(f"- resid {info['resid']:.3e}, xnorm {info['xnorm']:.6e}, the test's bound 8 (r + 4) u trace = {8 * (r + 4) * U * np.trace(Xk):.3e}")
    say()
    say("## EIG sources: reported residual against LAPACK on the same matrix")
    say()
    say("| case | cone | side | rank | resid (library, rocSOLVER dsyevd) | numpy's own `||Xk - (Xk)+||_F` | n u ||Xk||_F | ratio to the larger |")
    say("|---|---|---|---|---|---|---|---|")
    from kat_problems import sdp_wiki
    for name, prob, opt in (("full_eig_decomp = 1", pr, options(max_iter=400, full_eig_decomp=1)),
                            ("3 x 3 KAT (sdp_wiki)", sdp_wiki(False), options()),
                            ("equilibration_force = 1 (X = 0: the aliased scaling, status INFEASIBLE)", pr,
                             options(max_iter=400, equilibration_force=1)),
                            ("equilibration_force = 1, equilibration_reference_aliasing = 0", pr,
                             options(max_iter=400, equilibration_force=1, equilibration_reference_aliasing=0)),
                            ("3 x 3 KAT, equilibration_force = 1", sdp_wiki(False), options(equilibration_force=1))):
        s = B.solve(prob, opt, factors=True)
        for c in range(len(prob.psd)):
            v, V, i = s.psd_factors[c]
            X = block(s.primal, prob, c)
            w, Q = np.linalg.eigh(X)
            pos = w > 0
            own = float(np.linalg.norm(X - (Q[:, pos] * w[pos]) @ Q[:, pos].T))
            floor = X.shape[0] * U * float(np.linalg.norm(X))
            say(f"| {name} | {c} | {X.shape[0]} | {i['rank']} ({i['source_name']}) | {i['resid']:.3e} | {own:.3e} | {floor:.3e} | {i['resid'] / max(own, floor, 1e-300):.2f} |")
    say()

    # ---- 2. exit time on the bench instance
    n = args.n
    r0 = max(2, int(round(n ** 0.5)))
    prb = P.maxcut(n, seed=0)
    kw = dict(max_iter=args.iters, min_iter=args.iters, initial_target_rank=r0, max_target_rank_krylov_eigs=max(64, r0))
    B.solve(prb, options(**kw))                                             # warm-up: code objects, allocator
    plain, fact, srcs = [], [], None
    for _ in range(5):
        a = B.solve(prb, options(**kw))
        b = B.solve(prb, options(**kw), factors={0: args.cap})
        assert np.array_equal(a.primal, b.primal) and a.iter == b.iter
        plain.append(a.stats["exit_time"]); fact.append(b.stats["exit_time"])
        srcs = [f[2] for f in b.psd_factors]
        last = b
    say(f"## The bench instance: Max-Cut n = {n}, target rank pinned at {r0}, {args.iters} iterations, cap = {args.cap}")
    say()
    say(f"- `exit_time` of `proxsdp_hip_solve`: median {statistics.median(plain) * 1e3:.2f} ms of five ({', '.join(f'{t * 1e3:.2f}' for t in plain)})")
    say(f"- `exit_time` of `proxsdp_hip_solve_factored`: median {statistics.median(fact) * 1e3:.2f} ms of five ({', '.join(f'{t * 1e3:.2f}' for t in fact)})")
    say(f"- primal and iteration count of every pair of runs equal bit for bit; cones: " +
        ", ".join(f"{c}: {i['source_name']} rank {i['rank']}/{i['rank_found']} resid {i['resid']:.3e} xnorm {i['xnorm']:.4e}" for c, i in enumerate(srcs)))
    say()

    # ---- 3. kernel times on that solve's factors
    v, V, i = last.psd_factors[0]
    x = last.primal[prb.psd[0]]
    r2, x2, ms_res = B.factor_residual(x, n, V, v, repeat=args.repeat)
    _, ms_rec = B.reconstruct(V, v, n, repeat=args.repeat, mfma=1)
    N = n * (n + 1) // 2
    say(f"## Kernel event times at n = {n}, r = {len(v)} (mean of {args.repeat} launches)")
    say()
    say("| kernel | ms | 8 N bytes / time |")
    say("|---|---|---|")
    say(f"| `k_factor_residual` (reads the block) | {ms_res:.4f} | {8 * N / ms_res / 1e9:.2f} TB/s |")
    say(f"| `k_reconstruct_mfma<false>` (writes the block) | {ms_rec:.4f} | {8 * N / ms_rec / 1e9:.2f} TB/s |")
    say()
    say(f"(the entry's sums on these factors: resid {np.sqrt(r2):.3e}, xnorm {np.sqrt(x2):.6e})")
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text("\n".join(L) + "\n")


if __name__ == "__main__":
    main()
