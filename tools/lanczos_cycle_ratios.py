#!/usr/bin/env python3
"""Kernel / reference ratios of the per-cycle Lanczos checks (tests/lanczos_cycle_cases.py), one table row per case and cycle:
the rows of profiles/lanczos_cycles.md.  Needs a GPU.

    python tools/lanczos_cycle_ratios.py [OUT.md]
"""
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from proxsdp_jl_amd import binding as B          # noqa: E402

import lanczos_cycle_cases as L                  # noqa: E402


def rows(cs, A, packed, normA, cycles):
    o = B.default_options()
    for k, v in cs["opts"].items():
        B.set_option(o, k, v)
    got = B.lanczos_cycles(packed, cs["n"], cs["nev"], cycles, options=o)["cycles"]
    out, reuse, worst = [], None, 0.0
    for c, cy in enumerate(got):
        if cy["stop"]:
            cy = dict(cy, K=cy["K"] - 1)          # the steps in front of the one that stopped (no residual column behind it)
        Vr, alr, ber = L.reference_cycle(A, cy["V"], cy["kfirst"], cy["K"])
        qk, reuse = L.quantities(A, normA, cy, reuse)
        qr, _ = L.quantities(A, normA, dict(cy, V=Vr, alphas=alr, betas=ber), reuse)
        worst = max([worst] + [qk[q] / max(qr[q], L.EPS) for q in L.QUANTITIES])
        out.append(L.ratio_lines(cs["id"], c, cy, qk, qr) + (" stopped |" if cy["stop"] else " |"))
    return out, worst


def main():
    lines = ["| case | cycle | kfirst | K | engine and paths | " + " | ".join(L.QUANTITIES) + " | |",
             "|---|---|---|---|---|" + "---|" * (len(L.QUANTITIES) + 1)]
    worst = 0.0
    for cs in L.CASES:
        r, w = rows(cs, *L.matrix(cs["n"], cs["nev"]), cs["cycles"])
        lines += r
        worst = max(worst, w)
    for cs in L.STOP_CASES:
        r, w = rows(cs, *L.rank5_matrix(cs["n"]), 3)
        lines += r
        worst = max(worst, w)
    lines.append("")
    lines.append(f"largest ratio: {worst:.2f} (allowed: {L.MARGIN:g})")
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        pathlib.Path(sys.argv[1]).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
