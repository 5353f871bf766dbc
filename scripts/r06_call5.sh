#!/usr/bin/env bash
# Round 6, call 5: permute addressing of the M = 16 byte tables (q8_entry16: two half tables by sub-space parity) -- the whole GPU
# suite, then A/B numbers at 10M / 1.25M / 1M rows and k = 50 against call 2's (same boxes vary by ~1 %: both trees would have to run
# on one box for a fair A/B -- the previous tree's library is kept as libannlite_hip_prev.so and selected with ANNLITE_HIP_LIB).
set -u
cd "$(dirname "$0")/.."; OUT=gpurun_out/r06c5; mkdir -p $OUT
timeout 1200 python -m pytest tests -q -m gpu --maxfail=10 > $OUT/pytest_gpu.txt 2>&1; echo "suite rc=$?"; tail -8 $OUT/pytest_gpu.txt
A="--legs none --cpu-queries 0 --recall-queries 0 --no-rerank --warmup 20"
for lib in new prev new prev; do
  E=""; [ $lib = prev ] && E="ANNLITE_HIP_LIB=$PWD/annlite_amd/libannlite_hip_prev.so"
  for cfg in "10m --steps 100" "1250000 --rows 1250000 --steps 200 --streams 2" "1000000 --rows 1000000 --steps 200 --streams 2" "k50 --k 50 --steps 50 --streams 2"; do
    tag=${cfg%% *}; args=${cfg#* }
    env $E timeout 200 python bench.py --full $A $args 2>/dev/null | python -c "
import sys, json
d = json.loads([l for l in sys.stdin if l.startswith('{')][-1]); r = d['roofline']
print('%-5s %-8s q/s %9.0f ms/step %.4f kernel_ms %.4f frac %.3f at-clock %.3f (%s MHz) sha %s' % ('$lib', '$tag', d['value'], d['ms_per_step'], r['kernel_ms'], r['frac'], r.get('frac_at_measured_clock') or 0, int(r.get('shader_clock_mhz') or 0), d['result_sha256'][:8]))"
  done
done 2>&1 | tee $OUT/perm_addressing_ab.txt
