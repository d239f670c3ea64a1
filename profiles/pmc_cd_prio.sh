#!/bin/bash
# profiles/pmc_cd_prio.sh <tag> [passes] -- SQ counters of the two explicitly placed CD-solve kernels (cd_mfma_placed_kernel on
# the H side, cd_mfma64_placed_kernel on the W side) under `python bench.py --gpus 1`: rocprofv3 --pmc alone (no tracing option
# beside it), restricted to those kernels.  The library and, in an experiments build, the priority mode come from the
# environment (RCPPML_GPU_LIB_PATH, RCPPML_GPU_CD_PRIO).  passes = 1: all counters in one pass; 2: two passes, the normalising
# counters in both (rocprofv3 refuses a set that the hardware cannot collect at once).  Every pass runs under its own time limit
# and the script stops at the first one that fails.  Output: <out>/<tag>/summary.txt (out = $PMC_OUT, default build/pmc) -- per kernel the mean over its
# dispatches of every counter, and the shares of profiles/cd_prio_pmc.txt.
TAG=${1:-cd_prio}
PASSES=${2:-1}
REPO=$(pwd); OUT=${PMC_OUT:-$REPO/build/pmc}/$TAG; mkdir -p "$OUT"
BASE="GRBM_GUI_ACTIVE SQ_BUSY_CYCLES SQ_WAVE_CYCLES"
if [ "$PASSES" = 1 ]; then
    SETS=("$BASE SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAIT_INST_ANY")
else
    SETS=("$BASE SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU" "$BASE SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAIT_INST_ANY")
fi
cd /tmp && export TMPDIR=/tmp
i=0
for SET in "${SETS[@]}"; do
    i=$((i + 1))
    timeout -k 10 240 rocprofv3 --output-format csv --pmc $SET --kernel-include-regex 'cd_mfma(64)?_placed_kernel' -d "$OUT/p$i" -o sq -- \
        python $REPO/bench.py --gpus 1 > "$OUT/log$i.txt" 2>&1
    rc=$?
    if [ $rc -ne 0 ]; then echo "pass $i failed: rc $rc"; tail -20 "$OUT/log$i.txt"; exit $rc; fi
done
find "$OUT" -name "*.db" -delete
python $REPO/profiles/pmc_cd_prio_summary.py "$OUT" | tee "$OUT/summary.txt"
