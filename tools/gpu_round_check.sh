#!/bin/bash
# The round-end commands on one GPU box: full -m gpu suite, smoke(), the full bench (--full), rocprofv3 stats of the bench.
# usage (from the repo root): [OUT=<dir>] bash tools/gpu_round_check.sh <tag>   -> $OUT/<tag>_* (default OUT=out), prof.sh's profile
exec < /dev/null
TAG=${1:-final}
OUT=${OUT:-out}
mkdir -p $OUT
timeout 600 python -m pytest tests/ -x -q -m gpu -p no:cacheprovider > $OUT/${TAG}_tests.log 2>&1
echo "tests rc=$?"; grep -v "^Extension modules" $OUT/${TAG}_tests.log | tail -6
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1; echo "smoke rc=$?"; tail -3 $OUT/${TAG}_smoke.log
timeout 400 python bench.py --full --out $OUT/${TAG}_bench_full.json > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; echo "bench rc=$?"; cut -c1-400 $OUT/${TAG}_bench.json; tail -4 $OUT/${TAG}_bench.err
timeout 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29517 bench.py --gpus 1 --full --no-cpu-baseline --out $OUT/${TAG}_bench_torchrun_full.json > $OUT/${TAG}_bench_torchrun.json 2> $OUT/${TAG}_bench_torchrun.err; echo "torchrun bench rc=$?"; cut -c1-300 $OUT/${TAG}_bench_torchrun.json
PROF_TIMEOUT=240 bash tools/prof.sh $TAG 2>&1 | head -14
