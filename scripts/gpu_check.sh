#!/bin/bash
# One GPU-box visit: kernel parity, model parity, smoke, bench (+ rocprofv3 kernel stats).  Logs -> $LOG_DIR (default gpu_logs/).
# usage: scripts/gpu_check.sh [tests|kbench|bench|prof|dp2|all]
what=${1:-all}
export LOG_DIR=${LOG_DIR:-gpu_logs}
mkdir -p $LOG_DIR
export PYTHONUNBUFFERED=1
python - > $LOG_DIR/env.log 2>&1 <<'PY'
import torch, os
print('torch', torch.__version__, 'cuda', torch.cuda.is_available(), torch.cuda.get_device_name(0) if torch.cuda.is_available() else None)
p = torch.cuda.get_device_properties(0)
print('CUs', p.multi_processor_count, 'mem GB', p.total_memory / 2**30, 'host cores', os.cpu_count())
PY
cat $LOG_DIR/env.log
if [[ $what == tests || $what == all ]]; then
  timeout 1200 python -m pytest tests/test_gpu_kernels.py tests/test_gpu_bias.py tests/test_gpu_codec.py -m gpu -q --tb=short -n 4 --timeout 300 > $LOG_DIR/kernels.log 2>&1
  echo "kernels rc=$?"; tail -n 60 $LOG_DIR/kernels.log
  timeout 1200 python -m pytest tests/test_gpu_parity.py -m gpu -q --tb=short -s --timeout 600 > $LOG_DIR/parity.log 2>&1
  echo "parity rc=$?"; tail -n 80 $LOG_DIR/parity.log
  timeout 600 python __graft_entry__.py smoke > $LOG_DIR/smoke.log 2>&1
  echo "smoke rc=$?"; tail -n 5 $LOG_DIR/smoke.log
fi
if [[ $what == kbench || $what == all ]]; then
  timeout 600 python scripts/kbench.py > $LOG_DIR/kbench.log 2>&1
  echo "kbench rc=$?"; cat $LOG_DIR/kbench.log
fi
if [[ $what == bench || $what == all ]]; then
  timeout 900 python bench.py --full --steps 10 --warmup 3 > $LOG_DIR/bench.log 2>&1
  echo "bench rc=$?"; tail -n 12 $LOG_DIR/bench.log
fi
if [[ $what == dp2 ]]; then
  # two ranks sharing the one GPU over gloo: exercises bench.py's multi-rank control flow (per-layer bucket callbacks, barriers, the
  # instrumented step, the optimizer leg) on a 1-GPU box -- the numbers mean nothing
  ALM_BENCH_SHARE_GPU=1 timeout 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29511 \
    bench.py --gpus 2 --steps 3 --warmup 1 --full --no-cpu-baseline > $LOG_DIR/dp2.log 2>&1
  echo "dp2 rc=$?"; tail -n 3 $LOG_DIR/dp2.log | cut -c1-400
fi
if [[ $what == prof || $what == all ]]; then
  export TMPDIR=/tmp
  timeout 900 rocprofv3 --kernel-trace --stats -d $LOG_DIR/prof -o r1 -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-optimizer-leg > $LOG_DIR/prof.log 2>&1
  echo "prof rc=$?"; tail -n 5 $LOG_DIR/prof.log
  db=$(find $LOG_DIR/prof -name "*.db" | head -1)
  if [[ -n $db ]]; then python scripts/prof_summary.py "$db" $LOG_DIR/kernel_stats.csv "rocprofv3 --kernel-trace --stats -- python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-optimizer-leg (8 steps incl. warm-up + 1 instrumented)"; rm -f "$db"; head -n 30 $LOG_DIR/kernel_stats.csv | cut -c1-180; fi
fi
