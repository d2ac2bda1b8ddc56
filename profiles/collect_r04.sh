#!/bin/bash
# Round-4 profiles, on a GPU box, from the repo root:  bash profiles/collect_r04.sh OUT
# with OUT the folder profiles/tools/pmc_passes.sh writes under; then, on any machine:
#   python profiles/summarize_r04.py OUT
# Kernel-trace statistics of the bench command (a plain run: timed step only; --full: the whole line with every other
# config); then counter passes (one counter group per pass, --kernel-trace only, as
# MI355X_MICROARCH.md prescribes) over the dominant kernel of every BASELINE config that has one of
# its own: the headline CTC search (C2 shape), the C5 shard decode, the C3 search, C3 with the bigram
# model in the loop, C4 sparse_image_warp.
set -e
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
out=${1:?usage: bash profiles/collect_r04.sh OUT}/r04
mkdir -p "$out"
rocprofv3 --kernel-trace --stats -d "$out/bench_stats" -o bench --output-format csv -- \
  python3 bench.py --steps 10 --warmup 3 > "$out/bench_line.json" 2> "$out/bench.err"
echo "bench stats done"
rocprofv3 --kernel-trace --stats -d "$out/bench_full_stats" -o bench --output-format csv -- \
  python3 bench.py --full --steps 5 --warmup 2 --no-cpu-baseline > "$out/bench_full_line.json" 2> "$out/bench_full.err"
echo "bench full stats done"
bash profiles/tools/pmc_passes.sh r04/pmc_headline profiles/prof_ctc.py
bash profiles/tools/pmc_passes.sh r04/pmc_c5 profiles/prof_ctc_shape.py 512 4096 5000
bash profiles/tools/pmc_passes.sh r04/pmc_c3 profiles/prof_ctc_shape.py 1000 1024 1000
bash profiles/tools/pmc_passes.sh r04/pmc_lm profiles/prof_lm_table.py
bash profiles/tools/pmc_passes.sh r04/pmc_warp profiles/tools/time_warp.py
echo "all passes done"
