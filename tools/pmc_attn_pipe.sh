#!/bin/bash
# PMC passes over tools/pmc_attn.py for the pipelined attention kernels (default) and the one-chain kernels (pipe mode 0).
#   tools/pmc_attn_pipe.sh OUTDIR   -> one rocprofv3 directory + log per pass and counters.txt under OUTDIR
O=$(realpath -m "${1:?usage: tools/pmc_attn_pipe.sh OUTDIR}")
export TMPDIR=/tmp && cd "$(dirname "$0")/.." || exit 1
mkdir -p "$O"
P="rocprofv3 --output-format csv --kernel-trace"
for v in 1 0; do
  $P --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_BUSY_CYCLES SQ_ACTIVE_INST_ANY -d $O/pa_sq$v -o s -- python3 tools/pmc_attn.py $v > $O/pa_sq$v.log 2>&1
  $P --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_INSTS_SALU SQ_ACTIVE_INST_SCA -d $O/pa_lds$v -o s -- python3 tools/pmc_attn.py $v > $O/pa_lds$v.log 2>&1
done
rocprofv3 -L > $O/counters.txt 2>&1
echo done
