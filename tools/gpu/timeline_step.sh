# One forward+backward step as a kernel timeline: gpurun -- bash tools/gpu/timeline_step.sh
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
# output: $LCGS_PROFILE_OUT/tl2 (default profile_out/tl2)
O=${LCGS_PROFILE_OUT:-profile_out}/tl2
mkdir -p $O
rocprofv3 --kernel-trace --output-format csv -d $O/raw -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-train-step --no-stage-path --no-batch > $O/bench.json 2> $O/err.log
python3 profiles/timeline_step.py $O/raw > $O/timeline.txt 2>&1
rm -rf $O/raw
cat $O/timeline.txt
