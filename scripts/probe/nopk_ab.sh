# Round 5: the whole library built WITHOUT packed fp32 instructions (-Xclang -target-feature -Xclang -packed-fp32-ops; MI355X_MICROARCH: packed f32
# VALU beside MFMAs costs more than its issue slot) against the product library: C3 step, two rounds each, one box
O=${LG_OUT_DIR:-build/out}/r5q   # results folder (LG_OUT_DIR overrides its parent)
mkdir -p $O
for v in "" nopk "" nopk; do
  LG_LIB_VARIANT=$v timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/bench_${v:-product}_$RANDOM.json 2>/dev/null
done
for f in $O/bench_*.json; do python -c "
import json; d=json.loads(open('$f').read().strip().splitlines()[-1]); print('$f', d['ms_per_step'], d['value'], d['roofline']['frac'], d['clock']['in_kernel_mhz'])"; done
