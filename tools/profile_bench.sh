# The bench's rocprofv3 evidence: kernel stats of the loss-head bench, then FETCH_SIZE and
# WRITE_SIZE in separate PMC passes (never combined with tracing; each pass under its own limit).
# Outputs (small CSVs only): the kernel stats where tools/prof_stats.sh keeps them (prof_bench), the
# PMC passes under $OUT/pmc_fetch and $OUT/pmc_write (OUT defaults to profile_out).
# The bench's N = 1 loss_head_fp32 probe (--full) runs in every pass: the fp32 kernels (pair + hybrid
# A/B) are profiled and counted beside the bf16 one.
set -u
export TMPDIR=/tmp
OUT=${OUT:-profile_out}
B="bench.py --full --steps 47 --warmup 3 --no-cpu-baseline --no-trainer-step --no-c3"
P="bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-trainer-step --no-c3"
bash tools/prof_stats.sh prof_bench 240 $B || exit $?
for c in FETCH_SIZE WRITE_SIZE; do
  d=pmc_$( [ $c = FETCH_SIZE ] && echo fetch || echo write )
  mkdir -p $OUT/$d
  timeout -s KILL 150 rocprofv3 --pmc $c --output-format csv -d $TMPDIR/$d -o run -- python3 $P > $OUT/$d.log 2>&1 || exit $?
  find $TMPDIR/$d -name "*counter_collection.csv" -exec cp {} $OUT/$d/ \;
done
