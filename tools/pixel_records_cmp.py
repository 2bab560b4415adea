"""CPU side of tools/pixel_records_dump.py: the oracle's scattering steps of each dumped C4 pixel against the
device's records, step by step, with the comparator the suite uses (tests/records_compare.py compare_rows:
step sets, position and active count bit for bit, T sigma_s, every secondary ray's Tr, Li + Le against the row's
own Tr and against the oracle's). tests/test_gpu_records.py runs the same comparison on small frames without a
dump file.
    python3 tools/pixel_records_cmp.py TAG"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "3dg-vol-renderer_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"),
                os.path.join(ROOT, "tools")]
import numpy as np
import records_compare as RC
from fallback_sweep_local import c4_oracle_scene
from test_gpu_parity import LIGHTS_1000

tag = sys.argv[1]
d = np.load(os.path.join(ROOT, "gpurun_out", f"{tag}_records.npz"))
osc = c4_oracle_scene()
lp = np.float32([l[0] for l in LIGHTS_1000])
li = np.float32([l[1] for l in LIGHTS_1000])
for key in d.files:
    if key.endswith("_px"):
        continue
    x, y = (int(v) for v in key.split("_"))
    dev = d[key]
    orc = RC.oracle_rows(osc, x, y, 4096, 4096, dev.shape[1] - 9 - len(lp))
    rep = RC.compare_rows(dev, orc, lp, li, RC.ENV)
    print(f"== pixel ({x}, {y}): device {len(dev)} records, oracle {len(orc)}; pixel dev {d[key + '_px'].tolist()}")
    print(f"   {rep.summary()}")
    print("   " + rep.describe(limit=200).replace("\n", "\n   "))
