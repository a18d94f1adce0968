set -e
out=${1:?usage: tools/micro/gather_ab.sh <outdir>}; mkdir -p $out
timeout -k 10 500 python -m pytest tests/test_gather_gpu.py -x -q > $out/tests.log 2>&1
tail -3 $out/tests.log
for m in 1000000 125000; do for v in plain-gather plain; do
timeout -k 10 200 python bench.py --full --molecules $m --variant $v --steps 200 --no-extra --no-cpu-baseline > $out/b_${m}_$v.json 2>$out/b_${m}_$v.err || true
python - <<PY
import json
try:
    d=json.loads(open("$out/b_${m}_$v.json").read().strip().splitlines()[-1])
    print($m,"$v",round(d["value"],1),{k:v["avg_us"] for k,v in d["kernels"].items()})
except Exception as e: print("fail",e)
PY
done; done
