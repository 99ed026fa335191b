#!/bin/bash
# End-of-session check of the tree as committed: every GPU test, smoke(), the
# default bench line.  Stops at the first failing step.
R=${GRAFT_REPO_ROOT:-$(pwd)}
TAG=${1:-final}
mkdir -p "$R/bench_out"
cd "$R"
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 200 --timeout-method thread \
  > "bench_out/gpu_tests_$TAG.log" 2>&1 || { tail -30 "bench_out/gpu_tests_$TAG.log"; exit 1; }
tail -2 "bench_out/gpu_tests_$TAG.log"
timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke()" > "bench_out/smoke_$TAG.log" 2>&1 \
  || { tail -20 "bench_out/smoke_$TAG.log"; exit 1; }
tail -1 "bench_out/smoke_$TAG.log"
timeout -k 10 300 python bench.py --full > "bench_out/bench_$TAG.log" 2>&1 || { tail -20 "bench_out/bench_$TAG.log"; exit 1; }
tail -1 "bench_out/bench_$TAG.log" > "bench_out/bench_$TAG.json"
cut -c1-400 "bench_out/bench_$TAG.json"
