#!/bin/bash
# Per-kernel time of a single-triplet call (the reference's own calling pattern, back2future.lua:73-74), GPU box:
#   B2F_OUT=<dir> bash tools/b1_prof.sh [H W]   ->  $B2F_OUT/b1_kernel_stats_<H>x<W>.csv
H=${1:-1024}; W=${2:-1920}
R=${GRAFT_REPO_ROOT:?set GRAFT_REPO_ROOT}
O=${B2F_OUT:?set B2F_OUT to the directory the results go to}
cd /tmp && export TMPDIR=/tmp
rm -rf $O/b1prof
rocprofv3 --kernel-trace --stats -d $O/b1prof -o b1 --output-format csv -- python3 $R/bench.py --full --batch 1 --height $H --width $W --steps 20 --warmup 3 --no-extras --no-cpu-baseline --no-host-path > $O/b1prof_bench.json 2> $O/b1prof.err
find $O/b1prof -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $O/b1_kernel_stats_${H}x${W}.csv
find $O/b1prof -name "*kernel_trace.csv" | head -1 | xargs -I{} cp {} $O/b1_kernel_trace_${H}x${W}.csv
rm -rf $O/b1prof
cut -c1-100 $O/b1_kernel_stats_${H}x${W}.csv | head -5
