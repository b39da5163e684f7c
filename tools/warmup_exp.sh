# ms/step and the per-kernel split against the number of warm-up steps
# (DESIGN.md §7 "clock ramp"); run from the repository root, results in $OUT
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
for w in 5 20 80 300 5; do
  timeout -k 10 200 python bench.py --full --steps 20 --warmup $w --no-cpu-baseline --no-bcsr --no-reference-order --no-dense-baseline > "$OUT/wexp_$w.json" 2> "$OUT/wexp.err" || exit 3
  python -c "import json;d=json.load(open('$OUT/wexp_$w.json'));r=d['roofline'];print($w, round(d['ms_per_step'],4), round(r['kernel_ms'],4), round(r['step_parts_ms']['k_transpose'],4))"
done
