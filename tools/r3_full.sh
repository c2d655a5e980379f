#!/bin/bash
# Full GPU suite, smoke, then the driver-form bench with --full (cpu baseline + other configs).  Outputs under $OUT (default out/).
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}; mkdir -p "$OUT"; export TMPDIR=/tmp
python -c "import __graft_entry__ as g; g.build()" > "$OUT/build.log" 2>&1 || { tail -20 "$OUT/build.log"; exit 1; }
timeout -k 10 1000 python -m pytest tests -m gpu -q -x --timeout=400 > "$OUT/pytest_gpu.log" 2>&1
rc=$?; echo "pytest exit $rc" | tee -a "$OUT/pytest_gpu.log"
tail -8 "$OUT/pytest_gpu.log"
if [ $rc -ne 0 ]; then echo "PYTEST FAILED: skipping bench"; exit $rc; fi
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/smoke.log" 2>&1 || { echo "smoke failed"; tail -20 "$OUT/smoke.log"; exit 1; }
tail -2 "$OUT/smoke.log"
timeout -k 10 600 python bench.py --steps 20 --warmup 5 --full > "$OUT/bench_driver_form.log" 2>&1; echo "bench exit $?"
tail -1 "$OUT/bench_driver_form.log" | python -c "
import sys,json
d=json.loads(sys.stdin.read())
print('updates/s', round(d['value'],1), 'us/step', round(1e3*d['ms_per_step'],2), 'roofline', d['roofline'])
print('cpu', d['cpu_baseline'])
for k,v in d.get('other_configs',{}).items(): print(k, json.dumps(v))
"
