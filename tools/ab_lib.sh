# Same-box A/B of two builds of libf110qp.so (F110QP_LIB): bench.py kernel time per config,
# alternating the two libraries. Usage (GPU box): bash tools/ab_lib.sh PREV_SO "c2 c3 c5" [reps]
#   -> ${OUT_DIR:-out}/ab/
set -o pipefail
prev=$1; cfgs=$2; reps=${3:-2}
out=${OUT_DIR:-out}/ab
mkdir -p $out
for r in $(seq $reps); do
  for c in $cfgs; do
    for lib in cur prev; do
      if [ $lib = prev ]; then export F110QP_LIB=$prev; else unset F110QP_LIB; fi
      timeout -k 10 120 python bench.py --full --config $c --no-cpu --no-latency --steps 50 > $out/$c.$lib.json 2> $out/$c.$lib.err || exit 5
      python -c "import json;d=json.load(open('$out/$c.$lib.json'));print('$r $c $lib', '%.2f us'%(d['ms_per_step']*1e3), 'k %.2f'%(d['roofline']['kernel_ms_per_launch']*1e3))"
    done
  done
done
