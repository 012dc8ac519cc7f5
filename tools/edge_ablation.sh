# Edge-GEMM ablations inside the sampler (timing only; CHM_EDGE_DBG makes results wrong).
# Run from the repo root on the GPU box; results go to $OUT_DIR/abl (default out/abl).
O=${OUT_DIR:-out}/abl
mkdir -p $O
for d in ${ABL:-0 4 8 12 1}; do
  CHM_EDGE_DBG=$d timeout -k 10 240 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/d$d.json 2> $O/d$d.err || exit 1
done
