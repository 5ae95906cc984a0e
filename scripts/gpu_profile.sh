#!/bin/bash
# round profile of the bench command (bench.py --full): kernel-trace stats, then PMC passes (separate runs), summaries -> $OUT
set -u
TAG=$1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-profile_out}
rm -rf "$OUT/prof_$TAG" "$OUT/pmcb_$TAG"
mkdir -p "$OUT"
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof_$TAG" -- python bench.py --full --no-cpu-baseline > "$OUT/prof_$TAG.log" 2>&1
echo "stats exit $?"; grep '^{' "$OUT/prof_$TAG.log" | tail -1 | cut -c1-400
mkdir -p "$OUT/pmcb_$TAG"
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 400 rocprofv3 --pmc $c --kernel-trace --output-format csv -d "$OUT/pmcb_$TAG/$c" -- python bench.py --full --no-cpu-baseline --steps 20 --warmup 5 --spmv-reps 10 > "$OUT/pmcb_$TAG/$c.log" 2>&1
  rc=$?; echo "pmc $c exit $rc"; if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then exit $rc; fi
done
python scripts/pmc_traffic.py "$OUT/pmcb_$TAG" ${PMC_KERNEL:-spmv_rowblock_vcp_kernel} "$OUT/${TAG}_pmc_traffic.json"
cat "$OUT"/prof_$TAG/*/*_kernel_stats.csv | cut -c1-200
