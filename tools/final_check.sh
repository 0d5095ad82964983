set -e
# usage: tools/final_check.sh <outdir>   (from the repository root)
OUT=${1:?usage: tools/final_check.sh <outdir>}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest -x -q --timeout 200 --timeout-method thread -m gpu tests > "$OUT/tests.log" 2>&1
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/smoke.log" 2>&1
timeout -k 10 300 python bench.py --full > "$OUT/c2.log" 2>&1
timeout -k 10 200 python bench.py --full --config c3 --steps 3 --warmup 1 --no-cpu-baseline --no-serial > "$OUT/c3.log" 2>&1
timeout -k 10 200 python bench.py --full --config c5 --steps 3 --warmup 1 --no-cpu-baseline --no-serial > "$OUT/c5.log" 2>&1
