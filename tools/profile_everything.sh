#!/bin/bash
# Everything profiles/rNN/ holds, in one go on the GPU box (writes $PROFILE_OUT/r/, default profile_out/r/ in the repository):
# per-workload bench lines (compact line + the details file), rocprofv3 kernel stats and the seven PMC passes
# (tools/profile_all.sh), the default bench line, the in-batch loss kernels, and the small logs (clustered sweep, compute_loss
# probes, reference-batched passes, shard model, loop layouts).
R=$(cd "$(dirname "$0")/.." && pwd)
export PROFILE_OUT=$(realpath -m "${PROFILE_OUT:-$R/profile_out}")
O=$PROFILE_OUT/r
cd $R; mkdir -p $O
export WORKLOADS="${WORKLOADS:-fb15k237-transe fb15k237-distmult fb15k237-complex fb15k237-simple fb15k237-transe-clustered fb15k237-distmult-clustered fb15k237-transe-d768 wikidata5m-transe wikidata5m-complex wikidata5m-transe-f16 wikidata5m-complex-f16 wikidata5m-transe-block wikidata5m-complex-block wikidata5m-transe-full wikidata5m-complex-full wikidata5m-protocol}"
bash tools/profile_all.sh > $O/profile_all.log 2>&1
[ -n "$ONLY_WORKLOADS" ] && { ls $O; exit 0; }
python bench.py --full --steps 20 --warmup 5 --details $O/bench_default_details.json 2> $O/bench_default.stderr > $O/bench_default.json
bash tools/inbatch_profile.sh r/inbatch > $O/inbatch_profile.log 2>&1
python tools/inbatch_probe.py 2>&1 | grep "^inbatch" > $O/inbatch_probe.log
python tools/clustered_sweep.py 2>&1 | grep -v amdgpu > $O/clustered_sweep.log
python tools/loss_step_probe.py 2>&1 | grep -v "amdgpu\|^RCCL\|^HIP ver\|^ROCm\|^Hostname\|^Librccl" > $O/loss_step_probe.log
python tools/autograd_floor_probe.py 2>&1 | grep -v amdgpu > $O/autograd_floor_probe.log
python tools/queries_per_pass.py 2>&1 | grep -v amdgpu > $O/queries_per_pass.log
python tools/bench_batches.py 2>&1 | grep -v amdgpu > $O/bench_batches.log
python tools/wikidata_shard_model.py 2>&1 | grep -v amdgpu > $O/wikidata_shard_model.log
python tools/bench_small_blocks.py 2>&1 | grep -v amdgpu > $O/small_blocks.log
python -c "
import sys; sys.path.insert(0, '.')
from blp_amd import _lib
print('blp_selftest:', _lib.selftest(0)); print(_lib.device_caps(0))" 2>&1 | grep -v amdgpu > $O/selftest.log
BLP_BENCH_BACKEND=gloo python bench.py --gpus 8 --dry-nccl 2> $O/dry_nccl_8_gloo.stderr > $O/dry_nccl_8_gloo.json
BLP_BENCH_BACKEND=gloo python bench.py --gpus 8 --steps 2 --warmup 1 --full --details $O/bench_8_gloo_ranks_one_gpu_functional_details.json 2> $O/bench_8_gloo.stderr > $O/bench_8_gloo_ranks_one_gpu_functional.json
ls $O; du -sh $O
