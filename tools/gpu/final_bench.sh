# Final round bench lines: every leg (--full) with --acting, then the
# driver's own short plain command.
set -e
OUT=${OUT:-bench_out}   # results folder, relative to the repository root
mkdir -p $OUT
timeout -k 10 700 python bench.py --full --acting > $OUT/bench_final.json 2> $OUT/bench_final.err
python tools/bench_summary.py $OUT/bench_final.json | head -12
timeout -k 10 500 python bench.py --steps 20 --warmup 5 > $OUT/bench_driver.json 2> $OUT/bench_driver.err
python tools/bench_summary.py $OUT/bench_driver.json | head -3
