#!/bin/bash
# same-box A/B of one environment switch:  tools/dbg/ab_env.sh VAR valueA valueB OUTDIR   (per-shape listings and bench logs go to OUTDIR)
out=${4:?usage: tools/dbg/ab_env.sh VAR valueA valueB OUTDIR}
mkdir -p "$out"
for v in "$2" "$3" "$2" "$3"; do
  env $1=$v python bench.py --full --steps 8 --warmup 2 --no-cpu-baseline --shapes "$out/shapes_$1_$v.txt" > "$out/b_$v.log" 2>&1
  echo "$1=$v $(tail -1 "$out/b_$v.log" | cut -c60-140)"
done
