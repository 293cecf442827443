# Extends vln-ver_amd/tuning/tunableop_gfx950_vocc.csv with the GEMM shapes of the current bench.py defaults:
# TunableOp loads the existing table (file name + device ordinal), tunes the shapes it does not hold and writes the
# union back; merge $OUT/tunableop_next0.csv into the package table afterwards.
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
cd "$ROOT"
OUT=${OUT:-scratch/out}                 # where the logs and results go (kept out of git)
mkdir -p "$OUT"
cp vln-ver_amd/tuning/tunableop_gfx950_vocc.csv $OUT/tunableop_next0.csv   # TunableOp appends the device ordinal
export PYTORCH_TUNABLEOP_ENABLED=1
export PYTORCH_TUNABLEOP_FILENAME=$(cd "$OUT" && pwd)/tunableop_next.csv
export PYTORCH_TUNABLEOP_MAX_TUNING_DURATION_MS=15
export PYTORCH_TUNABLEOP_MAX_WARMUP_DURATION_MS=5
PYTORCH_TUNABLEOP_TUNING=1 timeout 2400 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-tuned-gemms ${BENCH_ARGS:-} > $OUT/tune.json 2> $OUT/tune.err; echo "tune $?"
wc -l vln-ver_amd/tuning/tunableop_gfx950_vocc.csv $OUT/tunableop_next*.csv; cut -c1-120 $OUT/tune.json; tail -2 $OUT/tune.err
