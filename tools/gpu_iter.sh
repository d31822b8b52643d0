# Usage: AM_OUT_DIR=<log directory> bash tools/gpu_iter.sh <tag>   -> <log directory>/<tag>/{tests.log,bench.out,bench.err}
OUT=${AM_OUT_DIR:?AM_OUT_DIR: the directory the logs go to}/$1
mkdir -p $OUT; timeout 900 python -m pytest tests/test_gpu_parity.py tests/test_gpu_configs.py -m gpu -x -q > $OUT/tests.log 2>&1; tail -3 $OUT/tests.log; python bench.py --full --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline > $OUT/bench.out 2> $OUT/bench.err; python - <<PY
import json
d=json.loads(open("$OUT/bench.out").read().strip().splitlines()[-1])
print("cfg3", d["value"], d["roofline"]["avg_launch_ms"])
for k,v in d["workloads"].items():
    if isinstance(v,dict): print(k, v["value"], v.get("count_only_gibps"), v["roofline"]["avg_launch_ms"], v.get("build_s"), v.get("host_results"))
PY
