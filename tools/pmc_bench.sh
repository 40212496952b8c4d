#!/bin/bash
# rocprofv3 --pmc passes over bench.py for one workload (one counter set per pass; FETCH_SIZE / WRITE_SIZE alone, as
# MI355X_MICROARCH.md prescribes), then the per-kernel summary -> profiles/.
# usage (on the GPU box):  tools/pmc_bench.sh <workload> <outdir: absolute, or a name under pmc_out/> [extra bench args]
W=$1; OUT=$2; shift 2
R=$(cd "$(dirname "$0")/.." && pwd)
# an absolute <outdir> is used as given; a relative one lands under pmc_out/ of the repository root (ignored by git)
case $OUT in /*) D=$OUT;; *) D=$R/pmc_out/$OUT;; esac
cd /tmp; export TMPDIR=/tmp
mkdir -p $D
i=0
for set in "FETCH_SIZE" "WRITE_SIZE" \
           "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_MFMA SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAIT_ANY SQ_WAIT_INST_ANY" \
           "GRBM_GUI_ACTIVE TCC_HIT_sum TCC_MISS_sum SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_CMD_FIFO_FULL SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VALU"; do
  i=$((i+1))
  rocprofv3 --pmc $set --output-format csv -d $D/pass$i -- python3 $R/bench.py --full --workload $W --layers 1 --steps 2 --warmup 1 \
      --prewarm-ms 0 --no-cpu-baseline --no-check --no-module --no-two-streams "$@" > $D/pass$i.log 2>&1
done
python3 $R/tools/pmc_traffic.py $D $W > $D/summary_$W.json
