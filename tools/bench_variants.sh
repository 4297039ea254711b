set -e
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 200 python bench.py --full --no-cpu-baseline > "$OUT/b_f32.json"
timeout -k 10 200 python bench.py --full --no-cpu-baseline --dtype f64 --steps 10 > "$OUT/b_f64.json"
timeout -k 10 200 python bench.py --full --no-cpu-baseline --quant uniform > "$OUT/b_u32.json"
timeout -k 10 200 python bench.py --full --no-cpu-baseline --quant uniform --dtype f64 > "$OUT/b_u64.json"
