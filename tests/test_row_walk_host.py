"""The code-object budget of the eight kernels that run the workgroup candidate walk (k_field_grid, k_point_cloud,
k_point_gradients, k_point_moments, k_particle_fields, k_neighbor_count, k_neighbor_fill, k_cc_hook), one table over all 32
instantiations (eight kernels x {float, double} x {2, 3}), read off the built library the way tests/test_bench_contract.py reads it.  No GPU.  The per-feature host
tests keep their own assertions; this one is the table a change to the walk — to one copy or to a shared one — is held to."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def walk_lds_bytes(row, box):
    """Two buffers of 256 staged rows of `row` doubles, the two range tables of a batch, four wave sums, and for the kernels that
    keep the box of their targets in an array of its own, 4 x 6 doubles."""
    return 2 * 256 * row * 8 + 2 * 256 * 4 + 4 * 4 + (4 * 6 * 8 if box else 0)


# kernel -> (doubles of a staged row, a box array of its own)
KERNELS = {
    "k_field_grid": (9, False),                                                     # 38928 bytes
    "k_point_cloud": (9, False),                                                    # 38928 (the box borrows the first staging buffer)
    "k_point_gradients": (9, False),                                                # the walk of k_point_cloud with 18 more sums
    "k_point_moments": (9, False),                                                  # ... with 24 more
    "k_particle_fields": (8, True),                                                 # 35024
    "k_neighbor_count": (4, True),                                                  # 18640
    "k_neighbor_fill": (4, True),
    "k_cc_hook": (4, True),
}

# registers of a lane: 128 leave four workgroups of four waves per compute unit.  k_point_moments is declared for two
# (__launch_bounds__(256, 2)) and with fp64 records takes 134 in 3-D, which still leaves three
REGISTER_CAP = {"k_point_moments<double, 3>": 134}


def test_every_instantiation_keeps_the_budget_of_the_walk(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_report
    from sphexample_amd import build
    assert [walk_lds_bytes(*KERNELS[k]) for k in ("k_field_grid", "k_particle_fields", "k_neighbor_count")] == [38928, 35024, 18640]
    co = isa_report.code_object(build.build(), str(tmp_path))
    meta = isa_report.metadata(co)
    names = isa_report.demangle(list(meta))
    seen = set()
    for kernel, (row, box) in KERNELS.items():
        mine = {names[k]: v for k, v in meta.items() if f"sphmi::{kernel}<" in names[k]}
        assert len(mine) == 4 and all(any(f"{kernel}<{t}, {d}>" in n for n in mine) for t in ("float", "double") for d in (2, 3)), (kernel, sorted(mine))
        for name, v in mine.items():
            assert v["scratch_bytes"] == 0, (name, v)
            assert v["max_flat_workgroup_size"] == 256, (name, v)
            assert v["lds_bytes"] == walk_lds_bytes(row, box), (name, v, walk_lds_bytes(row, box))
            assert 4 * v["lds_bytes"] <= 160 * 1024, (name, v)
            cap = next((c for k, c in REGISTER_CAP.items() if k in name), 128)
            assert v["vgprs"] + v["agprs"] <= cap, (name, v, cap)
            seen.add(name)
    assert len(seen) == 32
    # visitors and helpers are inlined: the code object holds kernels and nothing else
    outlined = [d for k, d in isa_report.demangle(list(isa_report.kernels(co))).items() if k not in meta]
    assert not outlined, outlined[:4]
