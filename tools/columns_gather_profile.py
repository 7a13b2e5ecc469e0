"""k_gather_columns at 1 057 738 rows x the seven-column set of RunSimulation (profiles/columns_on_device.md): five downloads in identity
order (right after the upload), five in developed order (c3_flowing after its rebuilds); yardstick: device-to-device copies of half the
bytes the gather moves (a copy of X bytes reads X and writes X), timed with events in this process.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o gather -- python tools/columns_gather_profile.py
    python tools/columns_gather_profile.py --parse OUT        → the k_gather_columns launches of the trace, in microseconds
"""
import csv, glob, json, os, sys, time


def parse(out_dir):
    rows = []
    for f in glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_gather_columns" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    us = [(b - a) / 1e3 for a, b in sorted(rows)]
    print(json.dumps({"k_gather_columns_us": us, "identity_us": us[:5], "developed_us": us[5:10]}))


if "--parse" in sys.argv:
    parse(sys.argv[sys.argv.index("--parse") + 1])
    sys.exit(0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import conftest
from test_columns_gpu import _seven, _like
from sphexample_amd.engine import make_engine

p, s = conftest.load_dam_break_3d_c3_flowing()
n = len(p)
eng = make_engine(p, s, device_float_bytes=4)
cols = _seven(p.ID)
eng.attach_columns(cols)
outs = _like(cols)
eng.pin(outs)
wall = {"identity": [], "developed": []}
def five(tag):
    for _ in range(5):
        t0 = time.perf_counter(); eng.download_columns(outs); wall[tag].append(time.perf_counter() - t0)
five("identity")
for a, b in zip(cols, outs):
    assert np.array_equal(a, b)
reb = 0
for steps in (20, 60, 60):
    reb = eng.advance(1e9, max_steps=steps).n_rebuilds
five("developed")
ids = eng.download(("ID",))["ID"]
for a, b in zip(_seven(ids), outs):
    assert np.array_equal(a, b)
moved_bytes = n * (96 + 81 + 8)
x = moved_bytes // 2
src = torch.empty(x, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(src); src.fill_(3)
torch.cuda.synchronize()
ms = []
for _ in range(7):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); dst.copy_(src); b.record(); torch.cuda.synchronize()
    ms.append(a.elapsed_time(b))
print(json.dumps({"N": n, "rebuilds": int(reb), "rows_moved": int((ids != p.ID).sum()), "gather_bytes_moved": moved_bytes, "copy_bytes": x,
                  "copy_ms": ms, "download_columns_wall_ms": {k: [1e3 * t for t in v] for k, v in wall.items()}}), flush=True)
eng.unpin(); eng.close()
