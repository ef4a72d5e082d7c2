#!/bin/bash
# Traffic behind the L2s (FETCH_SIZE / WRITE_SIZE, a pass of its own per counter, kernel trace only beside it) of the Lanczos
# step kernels at the metric's n = 4000, target rank 63, parent build and working tree in one job -> profiles/fop_owner.md
# section 4, profiles/pmc_traffic.json fop_step / 4000.
#   usage: tools/fop_owner_pmc.sh PARENT_TREE [OUT_DIR]     (from the repository root, both trees built)
set -o pipefail
export TMPDIR=/tmp
P=$(cd "$1" && pwd) || exit 2
R=$PWD
O=${2:-$R/build/fop_owner_pmc}; rm -rf "$O"; mkdir -p "$O"; O=$(cd "$O" && pwd)
CMD="python bench.py --steps 5 --warmup 2 --settle 20 --no-cpu --no-time-to-tol --no-packed-leg --no-early-leg --no-config-legs"
for side in parent new; do
  d=$R; [ $side = parent ] && d=$P
  for c in FETCH_SIZE WRITE_SIZE; do
    ( cd "$d" && timeout -k 10 240 rocprofv3 --pmc $c --kernel-trace -d "$O/${side}_$c" -- $CMD ) > "$O/${side}_$c.log" 2>&1
    rc=$?; echo "$side $c rc=$rc" | tee -a "$O/rc.txt"
    [ $rc = 0 ] || exit 1
    python tools/pmc_query.py "$O/${side}_$c" > "$O/${side}_$c.txt" 2>&1
    rm -rf "$O/${side}_$c"
    grep -E "k_lz_orth|k_fop" "$O/${side}_$c.txt"
  done
done
