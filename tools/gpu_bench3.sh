set -o pipefail
cd $GRAFT_REPO_ROOT
O=${OUT_DIR:-out}/k16b
mkdir -p $O
for i in 1 2 3; do timeout -k 10 200 python bench.py --full --steps 20 --warmup 5 --no-per-step --no-rollout --no-render --no-c3 --no-planner --no-cpu-baseline >> $O/headline.jsonl 2>> $O/headline.err || exit 1; done
timeout -k 10 400 python bench.py --full --no-cpu-baseline > $O/default.jsonl 2> $O/default.err || exit 1
