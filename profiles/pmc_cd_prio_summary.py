"""python profiles/pmc_cd_prio_summary.py DIR -- per kernel, the mean of every counter over the kernel's last 20 dispatches (the
timed iterations of bench.py) from the *_counter_collection.csv files rocprofv3 --pmc left under DIR (profiles/pmc_cd_prio.sh),
and the shares derived from them.  Units (rocprofv3's own derived metrics use the same): SQ_VALU_MFMA_BUSY_CYCLES counts cycles
per SIMD; SQ_ACTIVE_INST_VALU, SQ_WAVE_CYCLES and SQ_WAIT_INST_ANY count in units of four cycles; GRBM_GUI_ACTIVE is the
kernel's length in cycles, summed over the device's 8 XCDs (H-side kernel: 8.74e6 / 8 = 1.09e6 cycles = the 455 us of the
kernel trace at 2.4 GHz).  The base of the shares is GRBM_GUI_ACTIVE / 8 x SIMDs (4 per CU of the launch's grid: one workgroup
per CU), i.e. the time the kernel holds the SIMDs, tail included.  VALU-active counts the issue of every VALU instruction, the
MFMAs' own issue slots included; idle = 1 - MFMA-busy - VALU-active is therefore a lower bound of the time a SIMD issues
nothing."""
import collections
import csv
import glob
import os
import sys

XCDS = 8
acc = collections.defaultdict(lambda: collections.defaultdict(dict))
grid = {}
for path in sorted(glob.glob(os.path.join(sys.argv[1], "**", "*counter_collection.csv"), recursive=True)):
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(")[0].replace("void rk::", "")
        acc[name][r["Counter_Name"]][int(r["Dispatch_Id"])] = float(r["Counter_Value"])
        grid[name] = (int(r["Grid_Size"]), int(r["Workgroup_Size"]))
for name, ctrs in sorted(acc.items()):
    g, wg = grid[name]
    simds = 4 * (g // wg)
    print("%s   grid %d x %d threads = %d SIMDs, %d waves per SIMD" % (name, g // wg, wg, simds, wg // 256))
    m = {}
    for c, vals in sorted(ctrs.items()):
        ids = sorted(vals)[-20:]
        m[c] = sum(vals[i] for i in ids) / len(ids)
        print("   %-26s n=%d (of %d) mean %.6g" % (c, len(ids), len(vals), m[c]))
    if "GRBM_GUI_ACTIVE" in m:
        base = m["GRBM_GUI_ACTIVE"] / XCDS * simds
        line = ["kernel %.4g cycles" % (m["GRBM_GUI_ACTIVE"] / XCDS)]
        if "SQ_VALU_MFMA_BUSY_CYCLES" in m and "SQ_ACTIVE_INST_VALU" in m:
            mf, va = 100 * m["SQ_VALU_MFMA_BUSY_CYCLES"] / base, 100 * 4 * m["SQ_ACTIVE_INST_VALU"] / base
            line.append("MFMA-busy %.1f %%, VALU-active %.1f %%, idle %.1f %%" % (mf, va, 100 - mf - va))
        if "SQ_WAVE_CYCLES" in m:
            line.append("waves resident %.2f per SIMD" % (4 * m["SQ_WAVE_CYCLES"] / base))
        if "SQ_WAIT_INST_ANY" in m and "SQ_WAVE_CYCLES" in m:
            line.append("wave time waiting %.1f %%" % (100 * m["SQ_WAIT_INST_ANY"] / m["SQ_WAVE_CYCLES"]))
        if "SQ_INSTS_VALU" in m and "SQ_INSTS_LDS" in m:
            line.append("VALU per LDS instruction %.1f" % (m["SQ_INSTS_VALU"] / m["SQ_INSTS_LDS"]))
        print("   shares of GRBM_GUI_ACTIVE / 8 x SIMDs: " + ", ".join(line))
