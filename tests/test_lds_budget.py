"""The LDS and register budget of the bench's two neighbour kernels, read from the built code object (no GPU needed).

The window kernels (`k_neighbor_force<float, 3, 1|2, 33, 2, 2>`) hold per-lane pair queues and the own-row window in LDS, and nothing
else.  Their size decides how many four-wave workgroups a compute unit keeps: the header states the intended number next to the
`__shared__` arrays (`NeighborLds::kWorkgroupsPerCU`, a static_assert on the declared bytes); this holds the bytes the compiler really
allocated — rounded up to the block the device hands LDS out in — and the registers to the same occupancy."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LDS_PER_CU = 160 * 1024        # bytes of LDS per compute unit (gfx950)
LDS_BLOCK = 1280               # gfx950 allocates LDS in blocks of 320 dwords
VGPR_BLOCK = 8                 # registers per lane are allocated in eights, 512 per SIMD lane
VGPR_BUDGET = {"predictor": 72, "corrector": 80}
KERNELS = {"predictor": "k_neighbor_force<float, 3, 1, 33, 2, 2>", "corrector": "k_neighbor_force<float, 3, 2, 33, 2, 2>"}


def _intended_workgroups_per_cu():
    """The number the header's static_assert is written for (one four-wave workgroup = one wave on each SIMD)."""
    src = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_kernels.h")).read()
    m = re.search(r"kWorkgroupsPerCU\s*=\s*(\d+)\s*;", src)
    assert m, "NeighborLds::kWorkgroupsPerCU not found in sphmi_kernels.h"
    return int(m.group(1))


def _report():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    rep = isa_report.report(build.build(), list(KERNELS.values()))
    assert len(rep) == 2, sorted(rep)
    return {k: next(r for full, r in rep.items() if name in full) for k, name in KERNELS.items()}


def test_the_bench_kernels_keep_their_workgroups_per_compute_unit():
    wgs = _intended_workgroups_per_cu()
    assert 1 <= wgs <= 8
    for which, r in _report().items():
        assert r["scratch_bytes"] == 0, (which, r["scratch_bytes"])
        assert r["vgprs"] <= VGPR_BUDGET[which], (which, r["vgprs"])
        assert r["agprs"] == 0, (which, r["agprs"])
        allocated_vgprs = -(-r["vgprs"] // VGPR_BLOCK) * VGPR_BLOCK
        assert 512 // allocated_vgprs >= wgs, f"{which}: {r['vgprs']} registers leave fewer than {wgs} waves per SIMD"
        allocated_lds = -(-r["lds_bytes"] // LDS_BLOCK) * LDS_BLOCK
        assert allocated_lds * wgs <= LDS_PER_CU, f"{which}: {r['lds_bytes']} B of LDS ({allocated_lds} B allocated) x {wgs} workgroups exceed {LDS_PER_CU} B"
        assert r["max_flat_workgroup_size"] == 256, (which, r["max_flat_workgroup_size"])


def _header_geometry():
    """{"predictor" | "corrector": (entries, slack)} and the window's bytes, from NeighborLds in the header: `PASS == PASS_PREDICTOR ? p : c`."""
    src = open(os.path.join(ROOT, "sphexample_amd", "csrc", "sphmi_kernels.h")).read()
    geo = {}
    for field in ("kEntries", "kSlack"):
        m = re.search(field + r"\s*=[^;]*PASS == PASS_PREDICTOR \? (\d+) : (\d+)\s*;", src)
        assert m, f"NeighborLds::{field}: no per-pass literals found in sphmi_kernels.h"
        geo[field] = {"predictor": int(m.group(1)), "corrector": int(m.group(2))}
    win = int(re.search(r"kWinRecords\s*=\s*(\d+)\s*;", src).group(1)) * 32          # two 16-byte packets per record
    return {k: (geo["kEntries"][k], geo["kSlack"][k]) for k in KERNELS}, win


def test_the_bench_kernels_hold_queues_and_window_in_lds_and_nothing_else():
    """What the header's static_assert prices (queues + window) is ALL the code object allocates: four waves x 64 lanes x 8-byte entries x
    the header's depth for that pass, plus the window — to the byte.  An array added to these kernels without its line in NeighborLds
    would escape the compile-time budget, and shows up here."""
    geometry, win = _header_geometry()
    for which, r in _report().items():
        entries, slack = geometry[which]
        assert 4 <= entries <= 16 and 1 <= slack <= entries - 1, (which, entries, slack)
        assert r["lds_bytes"] == 4 * 64 * 8 * entries + win, (which, r["lds_bytes"], entries, win)
