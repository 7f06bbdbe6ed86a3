set -o pipefail
export TMPDIR=/tmp
OUT=${OUT:-evidence_out}; mkdir -p $OUT
for rep in 1 2; do
for a in "--arena" "--arena --placement plan" "" "--placement plan"; do
  timeout -k 10 240 python bench.py --full $a --steps 60 --warmup 10 --no-cpu-baseline --no-cold > $OUT/pl.json 2> $OUT/pl.err || { tail -5 $OUT/pl.err; exit 1; }
  python3 -c "import json; j=json.load(open('$OUT/pl.json')); r=j['roofline']; print('$a', j['value'], j['ms_per_step'], r['kernel_ms'], r['frac'])"
done; done
