set -e
O=${O:-out}
mkdir -p $O
timeout -k 10 400 python -m pytest tests -m gpu -x -q > $O/t.log 2>&1
timeout -k 10 200 python bench.py --full --steps 20 --warmup 3 --cpu-sample 0 > $O/b.log 2>&1
