#!/bin/bash
# Run ON THE GPU BOX (via gpurun): everything profiles/r04 is made of, from ONE box.  ~6 minutes.
set -u
ROOT=${GRAFT_REPO_ROOT:-$PWD}
cd "$ROOT" || exit 1
O=$ROOT/gpurun_out/r04
mkdir -p "$O"
export TMPDIR=/tmp
python tools/tuning/py_overhead2.py 2>&1 | grep -v amdgpu > "$O/py_overhead2.txt"
python bench.py --full > "$O/bench_n1.json" 2> "$O/bench_n1.err"; echo "bench rc=$?"
python bench.py --full --sweep --no-cpu --headline-only > "$O/bench_sweep.json" 2>> "$O/bench_n1.err"
TQ_BENCH_FORCE_DIST=1 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29544 \
    bench.py --gpus 1 --full --no-cpu > "$O/bench_rccl1.json" 2> "$O/bench_rccl1.err"; echo "bench rccl1 rc=$?"
bash scripts/profile_gpu.sh r04 > "$O/profile_gpu.log" 2>&1
bash scripts/profile_kernels.sh r04 > "$O/profile_kernels.log" 2>&1
python scripts/config_bench.py > "$O/config_bench.json" 2> "$O/config_bench.err"; echo "config_bench rc=$?"
tools/tuning/i8_v4 1 x > "$O/i8_v4_final.txt" 2>&1
timeout 1200 python -m pytest tests -q -m gpu -x -rs > "$O/gpu_tests_full_suite.log" 2>&1; echo "suite rc=$?"
tail -3 "$O/gpu_tests_full_suite.log"
head -c 1500 "$O/bench_n1.json"; echo
cat "$O/py_overhead2.txt"
