#!/bin/bash
# Round-3 evidence in ONE gpurun call: the driver's bench line, rocprofv3 kernel stats and PMC passes (separate passes per counter group,
# only with --kernel-trace) for all four legs of the path: forward / train step x fp32 / bf16-MLP.  Results under gpurun_out/r03;
# scripts/summarize_pmc.py reduces the PMC CSVs into profiles/ (run afterwards in the build container).  The program sits directly
# after `--`.   usage: bash scripts/collect_profiles_r03.sh [TAG]
ROOT=${GRAFT_REPO_ROOT:-/root/repo}
TAG=${1:-r03}
OUT=$ROOT/gpurun_out/$TAG
mkdir -p $OUT $ROOT/gpurun_out/pmc
cd $ROOT
python3 bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err && echo "bench (full record) done"
cd /tmp && export TMPDIR=/tmp
for leg in "fwd_f32:--mode forward --mlp f32 --steps 20 --warmup 3" "train_f32:--mode train --mlp f32 --steps 6 --warmup 2" "fwd_bf16:--mode forward --mlp bf16 --steps 40 --warmup 5" "train_bf16:--mode train --mlp bf16 --steps 10 --warmup 3" "split_fwd:--mode forward --split --steps 30 --warmup 4"; do
  name=${leg%%:*}; args=${leg#*:}
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT -o $name -- python3 $ROOT/bench.py $args --no-cpu-baseline --no-extra > $OUT/${name}_under_rocprof.json 2> $OUT/${name}_rocprof.err && echo "rocprof stats $name done"
  for pass in "FETCH_SIZE" "WRITE_SIZE" "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_INSTS_VALU_MFMA_MOPS_BF16 GRBM_GUI_ACTIVE" "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INST_CYCLES_VMEM SQ_VALU_MFMA_COEXEC_CYCLES"; do
    ptag=$(echo $pass | cut -d' ' -f1)
    rocprofv3 --pmc $pass --kernel-trace --output-format csv -d $ROOT/gpurun_out/pmc -o ${name}_$ptag -- python3 $ROOT/bench.py $args --steps 3 --warmup 1 --no-cpu-baseline --no-extra > $OUT/${name}_$ptag.bench.json 2> $OUT/${name}_$ptag.err || { echo "pmc pass $name $ptag failed"; tail -3 $OUT/${name}_$ptag.err; }
  done
  echo "pmc $name done"
done
rm -f $OUT/*_kernel_trace.csv $ROOT/gpurun_out/pmc/*_kernel_trace.csv $ROOT/gpurun_out/pmc/*agent_info.csv
ls $OUT | head -50
