#!/bin/bash
# One GPU session = the whole measurement loop: env info, per-kernel parity, model parity, bench, rocprof stats.
# Usage (on the GPU machine): [OUT=dir] bash tools/gpu_check.sh [quick|full|pmc]; results under $OUT (default out/)
mode=${1:-full}
R=$(cd "$(dirname "$0")/.." && pwd)
export OUT=$(realpath -m "${OUT:-$R/out}")      # results, the GPU tests' parity_report.txt included; absolute, since rocprofv3 runs from /tmp
cd "$R"
mkdir -p $OUT
exec > >(tee $OUT/gpu_check.log) 2>&1
echo "== host"; nproc; free -g | head -2; rocminfo | grep -E "Marketing|gfx|Compute Unit" | head -8
timeout -k 10 120 python -c "import torch;print(torch.__version__, torch.cuda.device_count(), torch.cuda.get_device_name(0))"
rm -f $OUT/parity_report.txt
echo "== kernel parity"; timeout 900 python -m pytest tests/test_gpu_kernels.py -m gpu -q --tb=short -p no:cacheprovider 2>&1 | tail -60
echo "== model parity"; timeout 1200 python -m pytest tests/test_gpu_model.py tests/test_gpu_dropin.py tests/test_gpu_preprocess.py tests/test_gpu_sampling.py -m gpu -q --tb=short -p no:cacheprovider > $OUT/model_parity.log 2>&1; tail -40 $OUT/model_parity.log | cut -c1-300
if [ "$mode" != "quick" ]; then
  echo "== smoke"; timeout 600 python __graft_entry__.py smoke 2>&1 | tail -5
  echo "== bench"; timeout 900 python bench.py --full --steps 3 --warmup 1 2>&1 | tail -5 | tee $OUT/bench.log
  echo "== bench fp8 B=1"; timeout 600 python bench.py --full --fp8 --steps 3 --warmup 1 --no-cpu-baseline 2>&1 | tail -1 | tee $OUT/bench_fp8.log
  echo "== bench sampled B=1"; timeout 600 python bench.py --full --sample --steps 3 --warmup 1 --no-cpu-baseline 2>&1 | tail -1 | tee $OUT/bench_sample.log
  echo "== bench B=64"; timeout 600 python bench.py --full --batch 64 --steps 1 --warmup 1 --no-cpu-baseline 2>&1 | tail -2 | tee $OUT/bench_b64.log
  echo "== kernel microbench"; (timeout 900 python tools/bench_kernels.py gemv1 vit 2>&1; VCLA_BENCH_MS=64 timeout 600 python tools/bench_kernels.py dstream 2>&1) | grep -v amdgpu.ids | tee $OUT/kernels.log
  echo "== rocprof B=64"; rm -rf $OUT/prof64; (cd /tmp && export TMPDIR=/tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof64 -o bench -- python $R/bench.py --full --batch 64 --steps 1 --warmup 1 --no-cpu-baseline 2>&1 | tail -1); f=$(find $OUT/prof64 -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -16 "$f" | cut -c1-200; find $OUT/prof64 -name "*kernel_trace.csv" -delete
  echo "== rocprof"; rm -rf $OUT/prof; cd /tmp && export TMPDIR=/tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o bench -- python $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline 2>&1 | tail -3
  cd "$R"; find $OUT/prof -name "*.csv" | head; f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && head -30 "$f"; find $OUT/prof -name "*kernel_trace.csv" -delete
fi
if [ "$mode" = "pmc" ]; then
  echo "== PMC (HBM traffic of the dominant kernel; separate passes, counters only)"
  for c in FETCH_SIZE WRITE_SIZE; do
    rm -rf $OUT/pmc_$c
    (cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc_$c -o pmc -- python $R/tools/pmc_gemv.py 2>&1 | tail -2)
    f=$(find $OUT/pmc_$c -name "*counter_collection.csv" | head -1)
    [ -n "$f" ] && python tools/pmc_summary.py "$f" $c gemv1p_kernel | tee $OUT/pmc_$c.txt
    find $OUT/pmc_$c -name "*.csv" -size +2M -delete
  done
  echo "== PMC MFMA utilisation of the 256x256 GEMM (LLaMA gate/up prefill shape)"
  timeout -k 10 120 rocprofv3 -L 2>/dev/null | grep -i -E "MFMA|GRBM_GUI_ACTIVE|SQ_BUSY_CYCLES|SQ_WAVE_CYCLES" | head -20 > $OUT/pmc_counters_available.txt; cat $OUT/pmc_counters_available.txt | cut -c1-160 | head -12
  for c in SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_BUSY_CYCLES; do
    rm -rf $OUT/pmcg_$c
    (cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --pmc $c --output-format csv -d $OUT/pmcg_$c -o pmc -- python $R/tools/pmc_gemm.py 2>&1 | tail -1)
    f=$(find $OUT/pmcg_$c -name "*counter_collection.csv" | head -1)
    [ -n "$f" ] && python tools/pmc_summary.py "$f" $c gemm_mfma256_kernel | tee $OUT/pmcg_$c.txt
    find $OUT/pmcg_$c -name "*.csv" -size +2M -delete
  done
fi
echo "== done"
