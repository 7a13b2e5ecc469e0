// sphmi_isosurface.h — the free surface as a mesh, extracted on the device from the Shepard sum of the lattice sampler
// (sphmi_isosurface_build): triangles in 3-D, a contour polyline in 2-D, of S = level on the lattice k_field_grid has just filled.
// What a node and a cell do — the Kuhn simplices, the edge and vertex rules, the element table, the arithmetic — is
// sphmi_iso_core.h, which a host program runs too; here are only the launches' bodies, one lane per node:
//   k_iso_classify   S at the node and at its 2^D − 1 upper neighbours → the mask of crossing edges it owns (one byte), their number,
//                    the inside set of the corners of the cell it names (one byte) and that cell's element count (0 on an upper face)
//   k_nl_tile_sums, k_nl_scan_tiles, k_nl_offsets (sphmi_neighbor_list.h, as they are), twice
//                    the two counts → int64 offsets [nodes + 1]; the totals are at most 7 · 2²⁴ and 12 · 2²⁴: they fit int32 indices
//   k_iso_vertices   every node its vertices, slot ascending, at voff[node] + rank, with the pressure and velocity means interpolated
//   k_iso_elements   every cell its elements at eoff[cell]; the index of an edge's vertex is voff[owner] + popcount(mask[owner] below
//                    the slot): no hash table, no atomics, the same bytes on every call
// Plain global loads: neighbouring lanes read neighbouring nodes (x fastest), the 2^D-fold reuse of S is left to the caches.  Per
// node the passes move 8 · 2^D bytes of S (mostly from cache), 10 bytes of masks and counts and 16 of offsets; per vertex 56 bytes
// out and up to 96 in.  profiles/isosurface.md has what that costs next to k_field_grid.
// No store leaves an array: a node past `nodes` does nothing, and the fill passes stop at the next node's offset.
#pragma once
#include <hip/hip_runtime.h>

#include "sphmi_iso_core.h"

namespace sphmi {

constexpr int kIsoThreads = 256;

template <int D> __global__ void __launch_bounds__(kIsoThreads) k_iso_classify(const IsoArgs A) {
    const long long node = (long long)blockIdx.x * kIsoThreads + (int)threadIdx.x;
    if (node < A.nodes) iso_classify_node<D>(A, (int)node);
}
template <int D> __global__ void __launch_bounds__(kIsoThreads) k_iso_vertices(const IsoArgs A) {
    const long long node = (long long)blockIdx.x * kIsoThreads + (int)threadIdx.x;
    if (node < A.nodes) iso_node_vertices<D>(A, (int)node);
}
template <int D> __global__ void __launch_bounds__(kIsoThreads) k_iso_elements(const IsoArgs A) {
    const long long node = (long long)blockIdx.x * kIsoThreads + (int)threadIdx.x;
    if (node < A.nodes) iso_cell_elements<D>(A, (int)node);
}

}  // namespace sphmi
