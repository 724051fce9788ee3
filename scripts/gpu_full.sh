#!/bin/bash
# the round-end sequence on one box: full GPU suite, smoke, bench.py --full (stops at the first failing step)
R=$(cd "$(dirname "$0")/.." && pwd); cd $R; mkdir -p out
timeout -k 10 1000 python -m pytest tests -m gpu -x -q > out/test_full.log 2>&1; rc=$?; echo "full gpu suite exit $rc"; tail -6 out/test_full.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > out/smoke.log 2>&1; rc=$?; echo "smoke exit $rc"; tail -2 out/smoke.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > out/bench_default.json 2> out/bench_default.err; rc=$?; echo "bench exit $rc"; [ $rc -eq 0 ] || exit $rc; python - <<'PY'
import json
d=json.loads(open("out/bench_default.json").read().strip().splitlines()[-1])
print(d["config"]["workload"][:60], d["value"], "Msamples/s", d["ms_per_step"], "ms; roofline frac", d["roofline"]["frac"], "hbm", d["roofline"]["hbm"]["frac"], "fetch", d["roofline"]["on_chip_fetch"]["frac"])
for k in ("pipelined","c2","c4","cpu_baseline"): print(k, d[k]["value"], d[k].get("ms_per_step"))
PY
