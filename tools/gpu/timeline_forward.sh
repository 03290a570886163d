# One forward-only frame as a kernel timeline (rocprofv3 --kernel-trace): gpurun -- bash tools/gpu/timeline_forward.sh
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
# output: $LCGS_PROFILE_OUT/tl (default profile_out/tl)
O=${LCGS_PROFILE_OUT:-profile_out}/tl
mkdir -p $O
rocprofv3 --kernel-trace --output-format csv -d $O/raw -- python3 bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-train-step --no-stage-path --no-backward --no-batch > $O/bench.json 2> $O/err.log

python3 profiles/timeline.py $O/raw > $O/timeline.txt 2>&1
rm -rf $O/raw
tail -60 $O/timeline.txt
