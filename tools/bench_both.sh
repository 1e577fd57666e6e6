#!/bin/bash
set -eu
R=${GRAFT_REPO_ROOT:?run this on the GPU box (gpurun sets GRAFT_REPO_ROOT)}
cd "$R"
# the two bench lines tools/file_bench.py files, both with every leg (--full): the default 200 steps and the short window
mkdir -p bench_out
timeout -k 10 900 python3 bench.py --full > bench_out/bench_full.json 2> bench_out/bench_full.err; echo "bench rc=$?"
timeout -k 10 600 python3 bench.py --full --steps 20 --warmup 5 > bench_out/bench_window.json 2> bench_out/bench_window.err; echo "window rc=$?"
