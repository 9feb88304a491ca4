#!/bin/bash
# Schur-gather experiments (round 3): XCD grouping x scene, kernel times from bench.py's HIP events and
# fabric traffic of k_schur_items from a FETCH_SIZE pass.  Run through gpurun from the repo root.
set -u
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$R/gpurun_out/${1:-exp_schur}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
BA="--no-cpu-baseline --no-matcher --no-d6 --no-mixed --no-pcg --no-dropin --no-driver-rows --no-alt-camera-solver --no-reference-order"
for grp in mod8 contig; do
  echo "== bench group=$grp"
  SFM_XCD_GROUP=$grp timeout -k 10 200 python3 $R/bench.py --full $BA > $OUT/bench_${grp}.json 2> $OUT/bench_${grp}.err || exit 1
done
for vis in random nearest; do for grp in mod8 contig; do
  echo "== pmc vis=$vis group=$grp"
  SFM_XCD_GROUP=$grp timeout -k 10 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/fetch_${vis}_${grp} -- python3 $R/bench.py --full --steps 2 --warmup 1 --visibility $vis --no-coherent $BA > $OUT/fetch_${vis}_${grp}.log 2>&1 || exit 1
  python3 $R/tools/pmc_summary.py k_schur_items $OUT/fetch_${vis}_${grp} > $OUT/fetch_${vis}_${grp}.txt
  find $OUT/fetch_${vis}_${grp} -name "*kernel_trace.csv" -delete
done; done
echo done
