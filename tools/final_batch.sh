# Five rocprofv3 passes, the bench lines, the micro-benchmarks, the power probe, on the GPU box:   bash tools/final_batch.sh r5 OUTDIR
# OUTDIR (relative to the repository root) = the directory tools/profile_round.sh and tools/power_probe.sh write into, where
# tools/collect_final.py reads the batch back.
set -o pipefail
TAG=${1:-r5}
OUT=${2:?usage: bash tools/final_batch.sh TAG OUTDIR}
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
bash tools/profile_round.sh ${TAG} 2>&1 | tail -8
python3 bench.py --full > "$OUT"/${TAG}_bench_final.json 2> "$OUT"/${TAG}_bench_final.err; tail -2 "$OUT"/${TAG}_bench_final.err
python3 bench.py --mode infer --res 512 --steps 20 --warmup 3 > "$OUT"/${TAG}_infer512_final.json 2>/dev/null
python3 bench.py --mode infer --res 256 --steps 20 --warmup 3 > "$OUT"/${TAG}_infer256_final.json 2>/dev/null
python3 bench.py --storage bf16 --train-res 512 --batch-gpu 8 --steps 16 --warmup 2 --no-cpu-baseline > "$OUT"/${TAG}_bench_bf16_512_final.json 2>/dev/null
python3 bench.py --storage bf16 --steps 16 --warmup 2 --no-cpu-baseline > "$OUT"/${TAG}_bench_bf16_final.json 2>/dev/null
python3 tools/bench_hbm_ops.py > "$OUT"/${TAG}_hbm_microbench.txt 2>/dev/null
python3 tools/bench_conv.py --reps 10 > "$OUT"/${TAG}_conv_microbench.txt 2>/dev/null      # (ends with the down-path section: fp32 tensor against operand pieces)
./tools/microbench/mfma_shape > "$OUT"/${TAG}_mfma_shape.txt 2>&1
python3 tools/phase_times.py > "$OUT"/${TAG}_phase_times.txt 2>&1 || true
echo BATCH1 DONE
# round-2 additions: the inference workload's per-kernel times, the chip's power / clock under the dominant kernel
export TMPDIR=/tmp
rm -rf "$OUT"/${TAG}_infer512_stats
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT"/${TAG}_infer512_stats -- python3 bench.py --mode infer --res 512 --no-cpu-baseline --steps 20 --warmup 2 > "$OUT"/${TAG}_infer512_stats.log 2>&1
find "$OUT"/${TAG}_infer512_stats -name "*.csv" ! -name "*kernel_stats.csv" -delete
bash tools/power_probe.sh "spade 256" > /dev/null 2>&1; cp gpurun_out/power_probe.txt gpurun_out/${TAG}_power_probe.txt
echo BATCH2 DONE
