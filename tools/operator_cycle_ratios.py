#!/usr/bin/env python3
"""Kernel / reference ratios of the per-cycle Lanczos checks on the operator form (tests/operator_cycle_cases.py), one table row
per case and cycle: the operator-form rows of profiles/lanczos_cycles.md.  Needs a GPU.

    python tools/operator_cycle_ratios.py [OUT.md]
"""
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import lanczos_cycle_cases as L                  # noqa: E402
import operator_cycle_cases as O                 # noqa: E402


def rows(cs, A, normA, got, tag=""):
    out, reuse, worst = [], None, 0.0
    for c, cy in enumerate(got["cycles"]):
        if cy["stop"]:
            cy = dict(cy, K=cy["K"] - 1)          # the steps in front of the one that stopped (no residual column behind it)
        Vr, alr, ber = L.reference_cycle(A, cy["V"], cy["kfirst"], cy["K"])
        qk, reuse = L.quantities(A, normA, cy, reuse)
        qr, _ = L.quantities(A, normA, dict(cy, V=Vr, alphas=alr, betas=ber), reuse)
        worst = max([worst] + [qk[q] / max(qr[q], L.EPS) for q in L.QUANTITIES])
        out.append(O.ratio_lines(cs["id"] + tag, c, cy, qk, qr) + (" stopped |" if cy["stop"] else " |"))
    return out, worst


def main():
    lines = ["| case | cycle | kfirst | K | engine and paths | " + " | ".join(L.QUANTITIES) + " | |",
             "|---|---|---|---|---|" + "---|" * (len(L.QUANTITIES) + 1)]
    worst = 0.0
    l2 = O.l2_case()
    for cs in O.CASES + ([l2] if l2 is not None else []):
        r, w = rows(cs, *O.operator(cs), O.capture(cs))
        lines += r
        worst = max(worst, w)
    for cs in O.WARM_CASES:
        r, w = rows(cs, *O.operator(cs), O.capture(cs, cycles=1, lanczos_warm_start=1), "-warm")
        lines += r
        worst = max(worst, w)
    for cs in O.STOP_CASES:
        pcs = O.rank5_pieces(cs["n"])
        r, w = rows(cs, O.Operator(cs["n"], pcs[0], pcs[1], pcs[3], pcs[4]), pcs[5], O.capture(dict(cs, cycles=3), pcs=pcs))
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
