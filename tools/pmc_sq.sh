#!/bin/bash
# SQ-level PMC passes over `bench.py` (separate passes, --kernel-trace only; see MI355X_MICROARCH.md "rocprofv3 PMC slots")
set -e
cd "${GRAFT_REPO_ROOT:-.}"
export TMPDIR=/tmp
OUT=gpurun_out/pmc_sq
mkdir -p $OUT
ARGS="--steps 10 --warmup 10 --no-cpu-baseline --no-also --full"
rocprofv3 -L > $OUT/counters_list.txt 2>&1 || true
rocprofv3 --kernel-trace --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_WAVES GRBM_GUI_ACTIVE --output-format csv -d $OUT/p1 -- python3 bench.py $ARGS > $OUT/p1.log 2>&1
echo pass1 done
rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_SALU --output-format csv -d $OUT/p2 -- python3 bench.py $ARGS > $OUT/p2.log 2>&1
echo pass2 done
rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_MISC SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_SCA SQ_INST_CYCLES_VMEM SQ_WAVE_CYCLES SQ_BUSY_CU_CYCLES --output-format csv -d $OUT/p3 -- python3 bench.py $ARGS > $OUT/p3.log 2>&1 || echo pass3 failed
echo pass3 done
find $OUT -name "*counter_collection.csv" | head
