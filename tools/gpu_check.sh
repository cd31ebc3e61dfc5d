#!/bin/bash
# One gpurun call: GPU test suite, bench (1 GPU; 1 rank with the data-parallel path forced), kernel profile.
# usage: tools/gpu_check.sh [tag] [log dir]       suite and bench logs -> <log dir>/<tag>_* (default build/logs); the kernel profile goes
# where tools/gpu_profile.sh writes it
tag=${1:-r02}
logs=${2:-build/logs}
mkdir -p "$logs"
export TMPDIR=/tmp
( timeout 1500 python -m pytest tests -q -m gpu --tb=short 2>&1 | tail -150 ) > "$logs/${tag}_pytest.log"
tail -60 "$logs/${tag}_pytest.log"
( timeout 600 python bench.py --full --steps 20 --warmup 5 2>&1 | grep '^{"metric"' ) > "$logs/${tag}_bench.log"
tail -c 3000 "$logs/${tag}_bench.log"
( ASR_FORCE_DDP=1 timeout 300 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline 2>&1 | grep '^{"metric"' ) > "$logs/${tag}_bench_ddp1.log"
tail -c 1500 "$logs/${tag}_bench_ddp1.log"
tools/gpu_profile.sh ${tag} 13 "python bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-roofline"
head -45 gpurun_out/${tag}_kernel_stats.txt
