set -e
O=${O:-out}
mkdir -p $O
timeout -k 10 400 python -m pytest tests -m gpu -x -q > $O/t.log 2>&1
timeout -k 10 200 python bench.py --full --steps 20 --warmup 3 --cpu-sample 0 > $O/b.log 2>&1
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
timeout -k 10 150 rocprofv3 --output-format csv --pmc FETCH_SIZE -d $O/pq/p3 -o run -- python3 bench.py --full --steps 2 --warmup 1 --cpu-sample 0 > $O/pq.log 2>&1
