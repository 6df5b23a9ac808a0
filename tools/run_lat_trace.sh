set -e
O=${O:-out}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p $O/lat
timeout -k 10 300 rocprofv3 --kernel-trace --memory-copy-trace --hip-runtime-trace --output-format csv -d $O/lat/tr -o run -- python3 bench.py --full --frames 512 --steps 2 --warmup 1 --cpu-sample 0 --latency-frames 60 --no-direct --no-stereo --no-bow --no-undistort --no-c4 --no-stage-timing > $O/lat/bench.json 2> $O/lat/bench.err
