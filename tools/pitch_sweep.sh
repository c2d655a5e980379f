#!/bin/bash
# headline step time and K3 launch time for several absolute row pitches of W / W_m (floats); logs under $OUT (default out/)
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}; mkdir -p "$OUT"; export TMPDIR=/tmp
python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || { tail -20 "$OUT/build.log"; exit 1; }
for p in "$@"; do
IMDBN_ROW_PITCH_ABS=$p timeout -k 10 200 python bench.py --steps 200 --warmup 20 --full --no-cpu-baseline --no-other-configs > "$OUT/bench_pitch_$p.log" 2>&1 || { echo "pitch $p failed"; tail -3 "$OUT/bench_pitch_$p.log"; continue; }
tail -1 "$OUT/bench_pitch_$p.log" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('pitch $p: us/step', round(1e3*d['ms_per_step'],2), 'K3 us', round(d['roofline']['avg_launch_us'],2))"
done
