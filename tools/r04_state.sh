#!/bin/bash
# Round-4 state check on the GPU box: GPU tests, then the bench lines - the driver's command first (its JSON carries `configs`:
# one decoder layer of c3 / c4 / c5), then one line per workload.   usage: tools/r04_state.sh <outdir under gpurun_out>
set -e
O=gpurun_out/$1; mkdir -p $O
python -m pytest tests -m gpu -x -q > $O/pytest.log 2>&1 || { tail -30 $O/pytest.log; exit 1; }
tail -3 $O/pytest.log
python bench.py --gpus 1 --steps 20 --warmup 5 > $O/bench_c2_driver.json 2> $O/bench_c2_driver.err
echo "driver line done"
python bench.py --full --no-configs > $O/bench_c2.json 2> $O/bench_c2.err
for w in c3 c4 c4row c5 d1 d16; do
  python bench.py --full --workload $w --no-cpu-baseline > $O/bench_$w.json 2> $O/bench_$w.err
  echo "$w done"
done
