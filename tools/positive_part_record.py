#!/usr/bin/env python3
"""profiles/positive_part.md from the lines tests/test_positive_part.py prints:

    python -m pytest tests/test_positive_part.py -m gpu -s -q > LOG
    python tools/positive_part_record.py LOG [OUT.md]

Every measured line of the log (prefix `PP|`) goes into the record unchanged, grouped by the test that printed it; the
header states the largest ratio of each group."""
import pathlib
import re
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
SIX = r"\| ((?:\d+\.\d+ ){5}\d+\.\d+) \|"


def lines_of(log, prefix):
    out = []
    for raw in log:
        line = re.sub(r"^\.*", "", raw)                      # (pytest -q prints its dots in front of a test's first line)
        if line.startswith(prefix):
            out.append(line[len(prefix):].strip())
    return out


def main():
    log = pathlib.Path(sys.argv[1]).read_text().splitlines()
    dst = pathlib.Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "profiles" / "positive_part.md"
    a, b, c, d = (lines_of(log, "PP|" + k) for k in "abcd")
    t, o = lines_of(log, "PP|time"), lines_of(log, "PP|obs")
    if not (a and b and c and d and t and o):
        sys.exit("the log lacks a group of lines: run the whole of tests/test_positive_part.py with -s")
    pa = max(float(x) for l in a for x in re.findall(r"= (\d+\.\d+)", l))
    pc = max(float(x) for l in c for x in re.findall(r"error / bound (\d+\.\d+)", l))
    pn = max(float(x) for l in d for x in re.findall(r"column npos \S+ / \S+ = (\d+\.\d+)", l))
    pd = max(float(x) for l in d for m in [re.search(SIX, l)] if m for x in m.group(1).split())
    out = ["# The positive-part Lanczos run and its certificate against exact checks (`proxsdp_hip_positive_part`)", "",
           "What `tests/test_positive_part.py` measures on one MI355X: the lines the tests print (`pytest -s`), unchanged, put together by",
           "`tools/positive_part_record.py`.  A ratio is the kernel's value over the plain fp64 NumPy reference's from the same inputs, both",
           "measured in long double; the tests allow 8 (floor 8 x 2^-52).",
           f"Largest ratios below: cycles {pa:.2f}; warm start {pc:.3f} of its bound; certificate: column npos {pn:.2f}, R1 - R3 {pd:.2f}.", "",
           "## a. Every cycle of a positive-part run", "",
           "| case | cycle | kfirst | K | engine | R1 all | R1 own | R2 all | R2 own | R3 alpha | R3 beta |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    out += a
    out += ["", "## b. What the run returns: true residuals (long double) against the thresholds the rule applied", "",
            "`tight`: two positive eigenvalues 5e-4 apart and an isolated first negative one, so that the positive pairs' tolerance decides --",
            "krylovkit_tol = 1e-12 needs a second cycle, `full_eig_lanczos_tol = 1e-9` accepts the first.", ""]
    out += ["- " + l for l in b]
    out += ["", "## c. The weighted warm start: column 0 against the long-double sum", "",
            "Error / bound: the bound is max(8 x the error of the same sum in plain fp64 NumPy, 8 x 2^-52 sum |terms|) per entry.", ""]
    out += ["- " + l for l in c]
    out += ["", "## d, e. The certificate", "",
            "Per case: the chunks `k_lz_measure<NCH>` was built for -> those of the last step kernels; column `npos` = (r2 - Z Z'r2) / |.|: error,",
            "kernel / reference; the six ratios R1 all, R1 own, R2 all, R2 own, R3 alpha, R3 beta of the columns npos .. npos + steps; theta_max;",
            "scale; mat-vecs.  `-own`: the certificate of a run's own result (e); `hazard`: the deficient start vector of the",
            "certified-projection test.", ""]
    out += ["- " + l for l in d]
    out += ["", "## Wall time per test (s, host side included)", ""]
    out += ["- " + l for l in t]
    out += ["", "## Observation: a small hidden positive eigenvalue (printed by `test_record_theta_max_on_a_small_hidden_eigenvalue`, not asserted)", "",
            "n = 257, ten steps; the locked pairs are all positive eigenvalues but one of tiny x 9; five matrices (seeds) per group.  The caller's",
            "test passes when theta_max <= 1e-6 x scale = 9e-6: ten steps do not promise to find a small isolated positive value.", "",
            "| tiny | npos | seed | hidden eigenvalue | theta_max (device) | theta_max (fp64 reference) | the caller's test |", "|---|---|---|---|---|---|---|"]
    out += o
    dst.write_text("\n".join(out) + "\n")
    print(f"{dst}: {len(a)} cycles, {len(b)} runs, {len(c)} warm starts, {len(d)} certificates, {len(o)} observations")


if __name__ == "__main__":
    main()
