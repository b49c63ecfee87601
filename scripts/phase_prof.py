"""Per-phase cycle breakdown of k_nodes (needs a -DDML_PHASE_PROF build via DML_HIP_LIB)."""
import ctypes, sys, runpy
import numpy as np
sys.argv = ["sweep_tiers.py"]
runpy.run_path("/root/repo/scripts/sweep_tiers.py", run_name="__main__")
from cs230_distributed_machine_learning_amd.utils import native
lib = native.hip_lib()
out = np.zeros(32, dtype=np.uint64)
lib.dml_forest_phase_stats.argtypes = [ctypes.c_void_p]
rc = lib.dml_forest_phase_stats(out.ctypes.data)
names = ["setup", "feat_extract", "hist", "eval", "select", "decision", "partition", "nodes"]
for t, tn in enumerate(["wave(64)", "block"]):
    v = out[t * 8:(t + 1) * 8].astype(float)
    n = v[7] or 1
    tot = v[:7].sum()
    rows = float(out[24 + t])
    print(tn, f"nodes={int(v[7])} rows/node={rows/n:.0f} cycles/node={tot/n:.0f}", "  ".join(f"{names[i]}={v[i]/n:.0f} ({100*v[i]/tot:.0f}%)" for i in range(7)))
print(f"block nodes of <= DML_PHASE_CHUNKS (default 4) chunks: {100 * float(out[27]) / max(1.0, out[8:15].astype(float).sum()):.1f}% of the block tier's cycles")
v = out[16:24].astype(float)
n = v[7] or 1
tot = v[:7].sum()
# the packed segmented evaluation (binary classification) splits its passes: slot 1 the pass set-up and
# the sort, 5 counting, scans and scores, 6 the selection; other builds keep everything in slot 1
sn = ["setup", "seg_sort", "onefeat_eval", "split_push", "tail", "seg_scan_score", "seg_select"]
print("subtree(64)", f"roots={int(v[7])} rows/root={float(out[26])/n:.1f} cycles/root={tot/n:.0f}",
      f"seg_eval={(v[1]+v[5]+v[6])/n:.0f} ({100*(v[1]+v[5]+v[6])/tot:.0f}%)",
      "  ".join(f"{sn[i]}={v[i]/n:.0f} ({100*v[i]/tot:.0f}%)" for i in (0, 1, 5, 6, 2, 3, 4)),
      f"seg_nodes={int(out[28])} (rows/node {float(out[29])/max(1,out[28]):.1f}) onefeat_nodes={int(out[30])} "
      f"(rows/node {float(out[31])/max(1,out[30]):.1f})")
