set -o pipefail
O=${O:-$(mktemp -d)}      # where this script keeps its logs and bench lines
V=$PWD/stroke-prediction_amd/lib/variants/nofront.so
SP_ZM_31=w8 timeout -k 10 600 python -m pytest tests/test_gpu_round3.py tests/test_gpu_round5.py tests/test_gpu_round2.py tests/test_gpu_bf16x3.py -x -q > $O/t.log 2>&1; tail -1 $O/t.log
for v in "X=1" "SP_ZM_31=w8" "X=1" "SP_ZM_31=w8"; do
  echo "== $v"; env "$v" timeout -k 10 200 python bench.py --full --steps 30 --warmup 5 --no-parity --no-cpu-baseline --no-secondary --layers > $O/b.out 2> $O/b.err; grep -E "conv_igemm  48->16" $O/b.err | cut -c1-100; python -c "import json; d=json.loads(open('$O/b.out').read().strip().splitlines()[-1]); print('ms', d['ms_per_step'], d['config'].get('loss'))"
done
for v in "SP_LIB_PATH=$V" "X=1" "SP_LIB_PATH=$V" "X=1"; do
  echo "== x3 ${v:0:12}"; env "$v" timeout -k 10 200 python bench.py --full --dtype bf16x3 --steps 30 --warmup 5 --no-parity --no-cpu-baseline --no-secondary --layers > $O/b.out 2> $O/b.err; grep -E "conv_igemm  (32->32 @60|16->32 @62|32->32 @48)" $O/b.err | cut -c1-75 | tr -s ' ' | tr '\n' '|'; echo;  python -c "import json; d=json.loads(open('$O/b.out').read().strip().splitlines()[-1]); print('x3 ms', d['ms_per_step'], d['config'].get('loss'))"
done
