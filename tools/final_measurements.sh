set -u
# Final measurements of the tree on one MI355X:  bash tools/final_measurements.sh OUTDIR
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
OUT=${1:?usage: bash tools/final_measurements.sh OUTDIR}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
# 1. driver-shaped bench line (all legs)
python bench.py --full --steps 20 --warmup 5 > $OUT/bench.json 2> $OUT/bench.err
# 2. per-launch CSV of a 5-step headline run
CALD_PROFILE_DUMP=$OUT/launches_fp32.csv python bench.py --steps 5 --warmup 2 > $OUT/bench5.json 2>/dev/null
# 3. whole-pool parity vs stored torch-CPU scores
python tools/parity_full_pool.py profiles/torch_cpu_reference_r2.npz $OUT/parity.json > $OUT/parity.log 2>&1
# 4. rocprof passes of the bench command
bash tools/profile_gpu.sh r6 > $OUT/profile.log 2>&1
# 5. training: kernel stats + event timeline + A/B of the pack plan
(cd /tmp && export TMPDIR=/tmp && rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/train_prof -o t -- python $ROOT/tools/bench_train.py --steps 20 --warmup 5 > $OUT/train_prof.log 2>&1)
rm -f $OUT/train_prof/*kernel_trace.csv
python tools/train_event_timeline.py > $OUT/train_timeline.txt 2>&1
tools/ab_train.sh "CALD_TRAIN_PACK_PLAN=0" "CALD_TRAIN_PACK_PLAN=1" 3 > $OUT/train_ab.txt 2>&1
python tools/bench_train.py --steps 30 --warmup 6 > $OUT/bench_train.json 2> $OUT/bench_train.err
python tools/bench_train.py --model retinanet --steps 30 --warmup 6 > $OUT/bench_train_retinanet.json 2>/dev/null
tail -c 600 $OUT/bench.json
