set -o pipefail
O=${O:-$(mktemp -d)}      # where this script keeps its logs and bench lines
for v in "SP_WGRAD_BIG_BLOCKS=0" "SP_WGRAD_BIG_BLOCKS=1" "SP_WGRAD_BIG_BLOCKS=2" "SP_WGRAD_BIG_BLOCKS=4" "SP_WGRAD_BIG_BLOCKS=0"; do
  echo "== $v"; env "$v" timeout -k 10 300 python bench.py --full --workload cae --steps 20 --warmup 5 --no-cpu-baseline --layers > $O/c.out 2> $O/c.err; grep -E "conv_wgrad  100->800" $O/c.err | cut -c1-100; python -c "import json; d=json.loads(open('$O/c.out').read().strip().splitlines()[-1]); print('ms', d['ms_per_step'], d['config'].get('loss'))"
done
timeout -k 10 600 python -m pytest tests/test_gpu_cae.py -x -q 2>&1 | tail -1
