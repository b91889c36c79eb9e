# tools/bench_full.sh OUTDIR -- the full bench (BASELINE metric config, every leg) + rocprofv3 evidence, into OUTDIR
set -e
OUT=${1:?usage: tools/bench_full.sh OUTDIR}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
export TMPDIR=${TMPDIR:-/tmp}
cd "$(dirname "$0")/.."
python3 bench.py --full > "$OUT/bench.json" 2> "$OUT/bench.err" || { tail -20 "$OUT/bench.err"; exit 1; }
cat "$OUT/bench.json"
# kernel-trace summary of the same workload: a plain run, the timed steps and nothing else
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/stats" -- python3 bench.py > "$OUT/stats.log" 2>&1 || tail -5 "$OUT/stats.log"
tail -2 "$OUT/stats.log"
find "$OUT/stats" -name "*kernel_stats.csv" -exec cat {} \;
PROF_READS=${PROF_READS:-50000000} bash tools/prof1.sh > "$OUT/prof.txt" 2>&1 || tail -20 "$OUT/prof.txt"
tail -60 "$OUT/prof.txt"
