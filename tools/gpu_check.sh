# GPU parity tests + default bench (+ optional extra bench args) on the GPU box; run from the repo root.
# Logs go to $OUT_DIR (default out/).
O=${OUT_DIR:-out}
mkdir -p $O
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $O/gputests.log 2>&1 || { tail -n 30 $O/gputests.log; exit 1; }
tail -n 2 $O/gputests.log
timeout -k 10 300 python -u bench.py --full --no-cpu-baseline "$@" > $O/bench.log 2>&1 || { tail -n 30 $O/bench.log; exit 1; }
python tools/bench_summary.py $O/bench.log
