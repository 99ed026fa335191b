# GPU tests + one bench line + batch-8 phase trace (for iterating on kernels).
set -e
mkdir -p bench_out
timeout -k 10 400 python -m pytest tests -m gpu -x -q > bench_out/gpu_tests.log 2>&1 || { tail -30 bench_out/gpu_tests.log; exit 1; }
tail -2 bench_out/gpu_tests.log
timeout -k 10 120 python bench.py --full --steps 300 --warmup 30 --no-cpu > bench_out/quick_bench.log 2>&1
tail -1 bench_out/quick_bench.log | python -c 'import json,sys; d=json.loads(sys.stdin.read()); print("fps", d["value"], "ms", d["ms_per_step"])'
timeout -k 10 120 python tools/trace_phases.py --batch 8 > bench_out/quick_trace.log 2>&1
cut -c1-100 bench_out/quick_trace.log | tail -16
