# rocprofv3 summary of the bench command (eager launches on one stream: graph-replayed kernels are not
# visible to --kernel-trace, and concurrent streams would overlap the per-kernel durations).  Run on the GPU box:
#     bash tools/profile_final.sh OUTDIR
# OUTDIR/prof_final_bench.json is the bench line (with its per-launch pass: --full) that tools/pmc_summarize.py reads.
O=$(realpath -m "${1:?usage: bash tools/profile_final.sh OUTDIR}") && mkdir -p "$O" || exit 1
R=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
export HSP_SERIAL_STREAMS=1   # the product step's own launches, one after the other on one stream
rm -rf "$O/prof_final"
rocprofv3 --kernel-trace --stats --output-format csv -d "$O/prof_final" -- python3 "$R/bench.py" --steps 5 --warmup 2 --no-graph --full --no-cpu-baseline --no-extra > "$O/prof_final.log" 2>&1
grep '^{' "$O/prof_final.log" | tail -1 > "$O/prof_final_bench.json"
find "$O/prof_final" -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} "$O/prof_final_kernel_stats.csv"
head -12 "$O/prof_final_kernel_stats.csv"
