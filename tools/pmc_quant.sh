#!/bin/bash
# PMC passes for the quantize kernel (separate rocprofv3 runs, counters only with --kernel-trace).
# usage: tools/pmc_quant.sh OUTDIR   (run from the repo root on the GPU box)
set -e
R=$PWD; OUT=$R/$1; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --pmc FETCH_SIZE -d $OUT/fetch -o p --output-format csv -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/fetch.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc WRITE_SIZE -d $OUT/write -o p --output-format csv -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/write.log 2>&1
timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT -d $OUT/sq -o p --output-format csv -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $OUT/sq.log 2>&1
echo done
