ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
cd "$ROOT"
OUT=${OUT:-scratch/out}                 # where the logs and results go (kept out of git)
mkdir -p "$OUT"
timeout 1500 python -m pytest tests -m gpu -x -q > $OUT/t_final.log 2>&1; echo "tests $?"; tail -3 $OUT/t_final.log
timeout 600 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -1
timeout 600 python bench.py --full > $OUT/b_final.json 2> $OUT/b_final.err; echo "bench $?"
python -c "
import json; d=json.load(open('$OUT/b_final.json')); print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline_other_kernels'][0]['frac'], d['cpu_baseline']['value'])"
