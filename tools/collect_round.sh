#!/bin/bash
# Everything the round's evidence needs, at the current HEAD, in one GPU call:
#   B2F_OUT=<dir> bash tools/collect_round.sh r04   ->  $B2F_OUT/profiles_r04/*, $B2F_OUT/sq_r04/*  (copy the summaries into profiles/)
TAG=${1:-r04}
R=${GRAFT_REPO_ROOT:?set GRAFT_REPO_ROOT}
O=${B2F_OUT:?set B2F_OUT to the directory the results go to}
cd $R
mkdir -p $O/profiles_$TAG
python3 bench.py --full > $O/profiles_$TAG/${TAG}_bench_default.json 2> $O/profiles_$TAG/bench_default.err
bash tools/collect_profiles.sh $TAG > $O/profiles_$TAG/collect.log 2>&1
bash tools/collect_sq.sh $TAG > $O/profiles_$TAG/collect_sq.log 2>&1
python3 tools/sq_summary.py $O/sq_$TAG $TAG >> $O/profiles_$TAG/collect_sq.log 2>&1
cp profiles/${TAG}_sq_counters.json $O/profiles_$TAG/ 2>/dev/null
bash tools/other_shapes.sh > $O/profiles_$TAG/${TAG}_other_shapes.txt 2>&1
ls -la $O/profiles_$TAG
