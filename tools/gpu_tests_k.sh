# GPU tests selected by a -k expression, then (optionally) the headline bench three times.
# Usage: [OUT_DIR=dir] bash tools/gpu_tests_k.sh TAG "<-k expr>" [bench]   (results under $OUT_DIR/TAG, default out/TAG)
set -o pipefail
cd $GRAFT_REPO_ROOT
TAG=${1:?tag}; EXPR=${2:?expr}
O=${OUT_DIR:-out}/$TAG
mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -k "$EXPR" \
  > $O/gputest.log 2>&1 || { echo PYTEST_FAILED; tail -30 $O/gputest.log; exit 1; }
tail -2 $O/gputest.log
if [ "$3" = bench ]; then
  for i in 1 2 3; do timeout -k 10 200 python bench.py --full --steps 20 --warmup 5 --no-per-step --no-rollout --no-render --no-c3 --no-planner --no-cpu-baseline >> $O/headline.jsonl 2>> $O/headline.err || exit 1; done
  timeout -k 10 400 python bench.py --full --no-cpu-baseline > $O/default.jsonl 2> $O/default.err || exit 1
fi
