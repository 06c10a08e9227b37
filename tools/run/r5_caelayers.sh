set -o pipefail
O=${O:-$(mktemp -d)}      # where this script keeps its logs and bench lines
SP_WGRAD_DEBUG=1 timeout -k 10 300 python bench.py --full --workload cae --steps 5 --warmup 2 --no-cpu-baseline --layers > $O/c.out 2> $O/c.err
grep -E "^wgrad " $O/c.err | sort -u | head -30
grep -E "conv_wgrad" $O/c.err | cut -c1-110 | sort -t@ -k2 | head -40
