# Per-kernel statistics including the stage-level operators: gpurun -- bash tools/gpu/kernel_stats.sh
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
# output: $LCGS_PROFILE_OUT/st (default profile_out/st)
O=${LCGS_PROFILE_OUT:-profile_out}/st
mkdir -p $O
rocprofv3 --kernel-trace --stats --output-format csv -d $O/raw -- python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-train-step --no-backward --no-batch > $O/bench.json 2> $O/err.log
python3 profiles/summarize.py $O/raw > $O/stats.txt 2>&1
rm -rf $O/raw
cat $O/stats.txt
