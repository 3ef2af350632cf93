#!/bin/bash
# Runs ON THE GPU BOX: the end-of-round record for the three profiled workloads (headline C3, C4 primal-dual, C5 shard) --
# kernel stats + the two PMC passes each -- and one `bench.py --full` run.   tools/collect_final.sh <tag> <out-dir>
# <out-dir> takes the logs and the bench line; tools/finish_final.sh reads it beside collect_profile.sh's <tag>_* folders.
# Then, in the build container:  tools/finish_final.sh <tag>   (summaries under profiles/, stamped with commit + source hash)
TAG=$1
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$(realpath -m "${2:?usage: tools/collect_final.sh <tag> <out-dir>}")
mkdir -p "$OUT"
bash "$ROOT/tools/collect_profile.sh" ${TAG}_c3 > "$OUT/collect_c3.log" 2>&1
bash "$ROOT/tools/collect_profile.sh" ${TAG}_pd --workload pd > "$OUT/collect_pd.log" 2>&1
bash "$ROOT/tools/collect_profile.sh" ${TAG}_c5 --size 8192 --bands 2 --dtype f64 > "$OUT/collect_c5.log" 2>&1
cd "$ROOT" && timeout -k 10 600 python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err"
tail -c 300 "$OUT/bench_default.json"
