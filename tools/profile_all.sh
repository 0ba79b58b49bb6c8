#!/bin/bash
# All bench workloads: bench JSON (with CPU baseline for the default workload) + tools/profile_round.sh
# summaries, under $PROFILE_OUT/r/<workload>/ (default profile_out/ in the repository).  Copy into profiles/rNN/ by hand.
R=$(cd "$(dirname "$0")/.." && pwd)
export PROFILE_OUT=$(realpath -m "${PROFILE_OUT:-$R/profile_out}")
OUT=$PROFILE_OUT
cd $R
mkdir -p $OUT/r
for w in ${WORKLOADS:-fb15k237-transe fb15k237-distmult fb15k237-complex fb15k237-simple fb15k237-transe-d768 wikidata5m-transe wikidata5m-complex wikidata5m-transe-block}; do
  mkdir -p $OUT/r/$w
  extra="--full --no-cpu-baseline --no-sub-results"
  [ "$w" = "fb15k237-transe" ] && extra="--full --no-sub-results"   # (the headline keeps its CPU baseline; the sub-results: the default run)
  python bench.py --workload $w --steps 10 --warmup 2 $extra --details $OUT/r/$w/bench_details.json 2> $OUT/r/$w/bench.stderr | tail -1 > $OUT/r/$w/bench.json
  bash tools/profile_round.sh --workload $w --no-hbm-probe > $OUT/r/$w/profile.log 2>&1
  cp $OUT/prof/kernel_stats.csv $OUT/prof/pmc*.csv $OUT/r/$w/ 2>/dev/null
  echo "$w done: $(cut -c1-160 $OUT/r/$w/bench.json)"
done
rm -rf $OUT/prof
du -sh $OUT/r
