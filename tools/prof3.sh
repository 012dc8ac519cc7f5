set -e
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=$R/${OUT_DIR:-out}/r5k
mkdir -p $O
for cfg in "512 40" "64 40" "64 20"; do
  set -- $cfg
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/p$1x$2 -o run --output-format csv -- python3 $R/bench.py --full --n-samples $1 --n-atoms $2 --steps 5 --warmup 2 --no-cpu-baseline --no-api-legs --no-traffic > $O/bench_$1x$2.json 2> $O/bench_$1x$2.err
done
