"""The dam_break_3d_c3 run of tools/examples_end_to_end.py (1 057 738 particles, t = 0 -> 0.4 s, 40 intervals, fp32, asynchronous output) on the
package of the tree given, so that two checkouts can be alternated in one job (profiles/columns_on_device.md): one JSON line.

    python tools/columns_end_to_end.py TREE 1|0        (1: with output, 0: without; $SPHMI_LIB picks the library)
"""
import copy, dataclasses, json, sys, time
root, with_output = sys.argv[1], sys.argv[2] == "1"
sys.path.insert(0, root)
from sphexample_amd.cases import dam_break_3d, setup_dam_break_3d
from sphexample_amd.simulation import RunSimulation
import sphexample_amd
s = setup_dam_break_3d(0.00425)
s = dataclasses.replace(s, SimMetaData=dataclasses.replace(s.SimMetaData, SimulationTime=0.4))
p = dam_break_3d(0.00425)
meta = copy.deepcopy(s.SimMetaData)
n_out = [0]
def on_output(md, P):
    n_out[0] += 1
t0 = time.perf_counter()
steps = RunSimulation(SimGeometry=None, SimMetaData=meta, SimConstants=s.SimConstants, SimKernel=s.SimKernel, SimParticles=p,
                      SimViscosity=s.SimViscosity, SimDensityDiffusion=s.SimDensityDiffusion, device_float_bytes=4,
                      on_output=on_output if with_output else None, async_output=True)
wall = time.perf_counter() - t0
print(json.dumps({"package": sphexample_amd.__file__, "with_output": with_output, "N": len(p), "wall_s": wall, "steps": int(meta.Iteration), "intervals": len(steps),
                  "outputs": n_out[0], "updates_per_s": len(p) * int(meta.Iteration) / wall, "chunk_ok": bool((p.ChunkID == 0).all())}), flush=True)
