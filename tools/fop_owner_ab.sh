#!/bin/bash
# Owner form of the operator-form Lanczos step against its parent build, alternating, in one job on one GPU
# (profiles/fop_owner.md): kernel trace of both builds, four plain bench pairs, output dumps compared.
#   usage: tools/fop_owner_ab.sh PARENT_TREE [OUT_DIR]      (from the repository root, both trees built)
# PARENT_TREE: a checkout of the parent commit with its own libproxsdp_hip.so.  Every GPU step has its own time limit and
# the script ends at the first step that fails.
set -o pipefail
P=$(cd "$1" && pwd) || exit 2
R=$PWD
O=${2:-$R/build/fop_owner_ab}; rm -rf "$O"; mkdir -p "$O"; O=$(cd "$O" && pwd)
run() { # name dir command...
  local name=$1 dir=$2; shift 2
  ( cd "$dir" && "$@" ) > "$O/$name.out" 2> "$O/$name.err"; local rc=$?
  echo "$name rc=$rc" | tee -a "$O/rc.txt"
  return $rc
}
TR="python bench.py --steps 20 --warmup 5"
for side in parent new; do
  d=$R; [ $side = parent ] && d=$P
  run kt_$side "$d" timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$O/kt_$side" -- $TR || exit 1
  python tools/prof_summary.py "$O/kt_$side" "$O/kernel_stats_$side.md" "kernel stats, $side build" "rocprofv3 --kernel-trace --stats -- $TR" > /dev/null || exit 1
  rm -rf "$O/kt_$side"
done
for p in 1 2 3 4; do
  run bench_parent_$p "$P" timeout -k 10 120 python bench.py || exit 1
  run bench_new_$p "$R" timeout -k 10 120 python bench.py || exit 1
done
run dump_parent "$P" timeout -k 10 120 python bench.py --dump-outputs "$O/dump_parent" || exit 1
run dump_new "$R" timeout -k 10 120 python bench.py --dump-outputs "$O/dump_new" || exit 1
python tools/compare_dumps.py "$O/dump_parent" "$O/dump_new" > "$O/compare_dumps.txt" 2>&1
rm -rf "$O/dump_parent" "$O/dump_new"
for p in 1 2 3 4; do
  for side in parent new; do
    python -c "import json,sys; a=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); r=a['roofline']; print(sys.argv[2], sys.argv[3], 'value %.2f' % a['value'], 'windows %.2f-%.2f' % tuple(a['config']['window_spread_it_per_s']), 'events: mat-vec %.3f us, orth %.3f us' % (1e3 * r['avg_matvec_launch_ms'], 1e3 * r['avg_orth_launch_ms']))" "$O/bench_${side}_$p.out" $p $side
  done
done
grep -E "k_lz_orth|k_fop" "$O/kernel_stats_parent.md" "$O/kernel_stats_new.md"
cat "$O/compare_dumps.txt"
