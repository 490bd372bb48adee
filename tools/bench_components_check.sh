# quick bench pass (tuning aid): print the components object of a short full bench run
# (output directory: $OUT, default bench_out)
export TMPDIR=/tmp
O=${OUT:-bench_out}
mkdir -p $O
timeout -k 10 300 python bench.py --full --steps 10 --no-cpu-baseline > $O/bc.json 2> $O/bc.err || { tail -20 $O/bc.err; exit 1; }
python3 -c "
import json; d=json.loads([l for l in open('$O/bc.json') if l.startswith('{')][0]); c=d['components']
for k in ('ntt_2^20_forward','poly_divide_zh_2^22','poly_eval_batch8_2^22','prove_2^20_gates'): print(k, c.get(k))"
