# two-stream timeline of the default bench step
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
export MMT_BENCH_NO_FP32_LEG=1
rm -rf $TMPDIR/pt
env ${EXTRA:-X=1} rocprofv3 --kernel-trace --output-format csv -d $TMPDIR/pt -- python $R/bench.py --full --no-cpu-baseline --steps 8 --warmup 3 --profile-steps 0 > $TMPDIR/b.json 2> $TMPDIR/err.txt
tail -1 $TMPDIR/b.json | cut -c1-160
python3 $R/mmt-psm_amd/tools/stream_timeline.py $(find $TMPDIR/pt -name "*kernel_trace.csv" | head -1) ${1:-}
