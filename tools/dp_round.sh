#!/bin/bash
# The data-parallel step on one GPU (world 1 over RCCL): bench line + kernel sequence with gaps.  Outputs under $OUT (default out/).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
ROOT=$PWD; OUT=${OUT:-out}; mkdir -p "$OUT"; OUT=$(cd "$OUT" && pwd); export TMPDIR=/tmp
python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || { tail -20 "$OUT/build.log"; exit 1; }
for m in factors allreduce; do
timeout -k 10 200 python bench.py --steps 200 --warmup 20 --full --no-cpu-baseline --no-other-configs --force-dp --dp-mode $m > "$OUT/bench_dp_$m.log" 2>&1 || { echo "bench $m failed"; tail -5 "$OUT/bench_dp_$m.log"; exit 1; }
tail -1 "$OUT/bench_dp_$m.log" | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$m: updates/s', round(d['value'],1), 'us/step', round(1e3*d['ms_per_step'],2), 'host enqueue us', round(d['host_enqueue_us_per_step'],1))"
done
rm -rf "$OUT/dpprof"
cd "$TMPDIR" && timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$OUT/dpprof" -- python3 "$ROOT/bench.py" --steps 30 --warmup 10 --no-cpu-baseline --no-other-configs --force-dp --no-k3-events > "$OUT/dpprof.log" 2>&1; echo "rocprof exit $?"
cd "$ROOT"; f=$(find "$OUT/dpprof" -name "*kernel_trace.csv" | head -1); python tools/trace_seq.py $f 36 > "$OUT/dp_seq.txt"; tail -30 "$OUT/dp_seq.txt"
