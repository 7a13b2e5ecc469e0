// sphmi_neighbor_list.h — the neighbour list of every row in CSR form, built on the device on demand (sphmi_neighbors_build).
//
// Row i, of any Type, lists every row j ≠ i of any Type with r² = ((dx² + dy²) + dz²) ≤ H² on the CURRENT positions — the cut of
// k_particle_fields (sphmi_particle_fields.h), formed the same way: from the doubles sphmi_download would deliver now (record + low
// word on fp32 handles), term by term with contraction off, inclusive, j = i excluded by row index, coincident rows listed.  A host
// reproduces it bit for bit from a download.  SPHMI_NEIGHBORS_HALF keeps j > i only: every pair once.
//
// Three passes, all on the engine's stream:
//   k_neighbor_count   one int32 per row
//   k_nl_tile_sums, k_nl_scan_tiles, k_nl_offsets
//                      an exclusive scan of the counts into int64 offsets[n + 1].  Every partial sum is 64 bits wide: at the per-device
//                      particle limit (2²⁷ rows) the total passes 2³¹.  REVIEWED, NOT EXERCISED: offsets beyond 2³¹ need more than 10⁷
//                      rows, more than a test can hold.
//   k_neighbor_fill    the same walk again; every lane appends the accepted j to the segment of its row
//
// The walk (nl_walk) is the candidate walk of k_particle_fields, copied: one workgroup of four waves takes 256 consecutive rows, one
// target per lane; the box of the run's targets widened by reach = H + h and the probes' 1e-6, clamped to the grid; per (cy, cz) the
// x-adjacent cells are one range of `cstart`, 256 ranges per batch, concatenated by a workgroup scan; chunks of 256 candidates are
// staged double buffered and every lane reads the staged rows in order (an LDS broadcast).  Its header derives why every target sees
// every row within H however stale the cell list.  Only what the cut needs is staged — x, y, z and the row index, 32 bytes per
// candidate instead of 64 — and nothing of the kernel sums is evaluated.
//   The candidates come in (cz, cy, row) order and the rows are sorted by cell, x fastest: the row index ascends along the walk.  A
//   lane therefore meets its neighbours in ascending j and APPENDS: no atomics decide an entry's place, the list of every row is
//   strictly ascending, and repeated calls write the same bytes.
//
// The fill pass's stores are the hot path: at 1.06 M rows with ≈150 neighbours each it writes 0.62 GB, every lane into a segment of
// its own about 600 bytes from its neighbour lane's.  It was built two ways and timed on that case (profiles/neighbor_list.md):
// one plain 4-byte store per accepted entry, and a buffer of 16 entries per lane in LDS flushed with 16-byte stores behind a scalar
// head up to the first 16-byte boundary of the segment.  The plain stores won — 26.5 ms against 28.3 ms, the count pass alone
// taking 26.9 ms: the walk, not the stores, bounds the pass.  (Inferred, not measured with counters: a lane's successive entries
// fall into the same cache line, which the L2 can complete before it leaves, while the buffer's LDS traffic and flush branch cost
// more than the wider stores save.)  The plain variant is the one kept.
//   No store leaves the segment: a lane stops appending at offsets[i + 1] (which the count pass, the same walk, makes exact).
//
// LDS: 2 × 256 staged rows of 32 bytes, the two range tables, the box — kNlLdsBytes, 18.25 KiB, under the 40 KiB that keep four
// workgroups per compute unit, the occupancy of k_particle_fields.  Lanes past N carry a NaN position: they fail every cut, count
// nothing and write nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_kernels.h"
#include "sphmi_rebuild.h"

namespace sphmi {

constexpr int kNlThreads = 256;                  // targets of a run, candidates of a chunk, ranges of a batch
constexpr int kNlRow = 4;                        // doubles of a staged row: x, y, z, row index (int64 bits)
constexpr size_t kNlLdsBytes = 2 * (size_t)kNlThreads * kNlRow * 8 + 2 * (size_t)kNlThreads * 4 + 4 * 6 * 8 + 64;      // of either kernel
static_assert(4 * kNlLdsBytes <= 160 * 1024, "four workgroups per compute unit");

constexpr int kNlScanThreads = 256, kNlScanItems = 8, kNlScanTile = kNlScanThreads * kNlScanItems;

template <class T> struct NeighborListArgs {
    using V4 = typename Vec4<T>::type;
    Half<const V4> pk0;                  // positions of the set sphmi_download reads
    const V4* comp;                      // fp32 handles: low words of position and density (null: none)
    const int* cstart;
    int* counts;                         // [N]      written by k_neighbor_count
    const long long* offsets;            // [N + 1]  read by k_neighbor_fill
    int* neighbors;                      // [offsets[N]]
    GridDesc g;
    double H_inv, H2, reach;
    int N, half;
};

// The candidate walk for the 256 rows of this workgroup: calls accept(j) on the lane of target i for every row j within the cut, in
// ascending j.  `i`: the row of this lane; `has_row`: i < N.
template <class T, int D, class Accept>
__device__ __forceinline__ void nl_walk(const NeighborListArgs<T>& A, const long long i, const bool has_row, Accept&& accept) {
    using V4 = typename Vec4<T>::type;
    __shared__ double s_row[2][kNlThreads * kNlRow];
    __shared__ int s_rs[kNlThreads], s_incl[kNlThreads];
    __shared__ double s_box[4][6];
    __shared__ int s_wave[4];
    static_assert(sizeof(s_row) + sizeof(s_rs) + sizeof(s_incl) + sizeof(s_box) + sizeof(s_wave) <= kNlLdsBytes, "LDS of the neighbour-list walk");
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const double kNaN = __longlong_as_double(0x7ff8000000000000ll);

    double xi[3] = {kNaN, 0.0, 0.0};
    if (has_row) {
        const V4 q0 = A.pk0[i];
        V4 lw; lw.x = lw.y = lw.z = lw.w = T(0);
        if (sizeof(T) == 4 && A.comp) lw = A.comp[i];
        xi[0] = (double)q0.x + (double)lw.x; xi[1] = (double)q0.y + (double)lw.y; xi[2] = D == 3 ? (double)q0.z + (double)lw.z : 0.0;
    }

    // the box of the run's targets (a lane without a row takes no part), then its cell span, padded and clamped like a probe's
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool empty = false;
    {
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        double bmin[3], bmax[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            bmin[d] = has_row ? xi[d] : inf; bmax[d] = has_row ? xi[d] : -inf;
            if (d >= D) continue;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { bmin[d] = fmin(bmin[d], __shfl_xor(bmin[d], o, 64)); bmax[d] = fmax(bmax[d], __shfl_xor(bmax[d], o, 64)); }
        }
        if (lane == 0) {
#pragma unroll
            for (int d = 0; d < 3; ++d) { s_box[wave][d] = bmin[d]; s_box[wave][3 + d] = bmax[d]; }
        }
        __syncthreads();
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (d >= D) continue;
            const double xf = fmin(fmin(s_box[0][d], s_box[1][d]), fmin(s_box[2][d], s_box[3][d]));
            const double xl = fmax(fmax(s_box[0][3 + d], s_box[1][3 + d]), fmax(s_box[2][3 + d], s_box[3][3 + d]));
            double a = (xf - A.reach) * A.H_inv, b = (xl + A.reach) * A.H_inv;
            a -= 1e-6 * (1.0 + fabs(a)); b += 1e-6 * (1.0 + fabs(b));
            const double off = 1.0 - (double)A.g.gmin[d], top = (double)(A.g.np[d] - 1);
            const double l = fmax(ceil(a - 0.5) + off, 0.0), u = fmin(floor(b + 0.5) + off, top);
            if (!(l <= u)) empty = true;                        // (a NaN coordinate lands here too)
            lo[d] = empty ? 0 : (int)l; hi[d] = empty ? 0 : (int)u;
        }
    }
    const int ny = hi[1] - lo[1] + 1, nz = D == 3 ? hi[2] - lo[2] + 1 : 1;
    const int nrange = empty ? 0 : ny * nz;

    for (int rbase = 0; rbase < nrange; rbase += kNlThreads) {
        // range rbase + t = (cy, cz): its x-adjacent cells are one range of rows
        int rs = 0, rc = 0;
        if (rbase + t < nrange) {
            const int r = rbase + t;
            const int cy = lo[1] + r % ny, cz = D == 3 ? lo[2] + r / ny : 0;
            const int row = A.g.np[0] * (cy + A.g.np[1] * cz);
            rs = A.cstart[row + lo[0]];
            rc = A.cstart[row + hi[0] + 1] - rs;
            if (rs < 0 || rc < 0 || rs + rc > A.N) { rs = 0; rc = 0; }      // (cannot happen on a consistent cell list; keeps every load inside the arrays)
        }
        // the ranges concatenated: candidate q of the batch lies in the first range whose inclusive scan exceeds q
        int incl = rc;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
        __syncthreads();                                    // the batch before is walked: its tables and buffers are free
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += s_wave[w];
        s_rs[t] = rs - (incl - rc);                          // candidate q of this range is row s_rs + q
        s_incl[t] = incl;
        __syncthreads();
        const int total = s_incl[kNlThreads - 1];
        const int nchunk = (total + kNlThreads - 1) / kNlThreads;

        V4 q0, lw;
        int k = 0;
        auto load = [&](int c) {
            const int q = c * kNlThreads + t;
            k = 0;
            if (q < total) {
                int a = 0, b = kNlThreads - 1;               // the first range with s_incl > q
                while (a < b) { const int m = (a + b) >> 1; if (s_incl[m] > q) b = m; else a = m + 1; }
                k = s_rs[a] + q;
            }
            q0 = A.pk0[k];
            if (sizeof(T) == 4 && A.comp) lw = A.comp[k]; else { lw.x = lw.y = lw.z = lw.w = T(0); }
        };
        auto stage = [&](int buf) {                          // (a lane past `total` stages row 0 again: the walk stops at `total`)
            double* r = &s_row[buf][t * kNlRow];
            r[0] = (double)q0.x + (double)lw.x;
            r[1] = (double)q0.y + (double)lw.y;
            r[2] = (double)q0.z + (double)lw.z;
            r[3] = __longlong_as_double((long long)k);
        };
        if (nchunk > 0) { load(0); stage(0); }
        __syncthreads();
        for (int c = 0; c < nchunk; ++c) {
            const bool more = c + 1 < nchunk;
            if (more) load(c + 1);                           // in flight while chunk c is walked
            const double* R = s_row[c & 1];
            const int cnt = min(kNlThreads, total - c * kNlThreads);
#pragma unroll 2
            for (int j = 0; j < cnt; ++j) {
                const double* r = R + j * kNlRow;
                double r2;
                {
                    // (no contraction: r² is ((dx² + dy²) + dz²) rounded term by term, as in k_particle_fields)
#pragma clang fp contract(off)
                    const double dx = xi[0] - r[0], dy = xi[1] - r[1], dz = D == 3 ? xi[2] - r[2] : 0.0;
                    r2 = dx * dx + dy * dy + dz * dz;
                }
                if (r2 <= A.H2) {
                    const long long row = __double_as_longlong(r[3]);
                    if (A.half ? row > i : row != i) accept((int)row);
                }
            }
            if (more) stage((c + 1) & 1);                    // the buffer chunk c − 1 was walked from: every lane is past the barrier behind it
            __syncthreads();
        }
    }
}

template <class T, int D>
__global__ void __launch_bounds__(kNlThreads, 4) k_neighbor_count(const NeighborListArgs<T> A) {
    const long long i = (long long)blockIdx.x * kNlThreads + (int)threadIdx.x;
    const bool has_row = i < (long long)A.N;
    int n = 0;
    nl_walk<T, D>(A, i, has_row, [&](int) { n += 1; });
    if (has_row) A.counts[i] = n;
}

template <class T, int D>
__global__ void __launch_bounds__(kNlThreads, 4) k_neighbor_fill(const NeighborListArgs<T> A) {
    const long long i = (long long)blockIdx.x * kNlThreads + (int)threadIdx.x;
    const bool has_row = i < (long long)A.N;
    long long pos = 0, end = 0;                              // the next entry of this lane's segment that is not written; its end
    if (has_row) { pos = A.offsets[i]; end = A.offsets[i + 1]; }
    int* const out = A.neighbors;
    nl_walk<T, D>(A, i, has_row, [&](int j) {
        if (pos >= end) return;                              // (cannot happen: the count pass ran this walk)
        out[pos] = j; pos += 1;
    });
}

// ---- the scan: counts (int32) → offsets (int64), exclusive, offsets[n] = the total ------------------------------------------------
// tile sums → their exclusive scan in place (one workgroup) → the offsets of every tile.  Every sum is a long long.
__global__ void __launch_bounds__(kNlScanThreads) k_nl_tile_sums(const int* __restrict__ counts, int n, long long* __restrict__ tsum) {
    __shared__ long long s_w[kNlScanThreads / 64];
    const int t = (int)threadIdx.x;
    const long long base = (long long)blockIdx.x * kNlScanTile + (long long)t * kNlScanItems;
    long long s = 0;
#pragma unroll
    for (int e = 0; e < kNlScanItems; ++e) if (base + e < n) s += counts[base + e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((t & 63) == 0) s_w[t >> 6] = s;
    __syncthreads();
    if (t == 0) { long long a = 0; for (int w = 0; w < kNlScanThreads / 64; ++w) a += s_w[w]; tsum[blockIdx.x] = a; }
}

// the exclusive scan of a workgroup's values in 64 bits; s_w: one slot per wave
__device__ __forceinline__ long long nl_block_exclusive(long long v, long long* s_w, long long& block_total) {
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6, nw = (int)blockDim.x >> 6;
    long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const long long u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    __syncthreads();                                         // (s_w of an earlier call is read)
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    long long before = 0, all = 0;
    for (int w = 0; w < nw; ++w) { const long long x = s_w[w]; if (w < wave) before += x; all += x; }
    block_total = all;
    return before + incl - v;
}

__global__ void __launch_bounds__(1024) k_nl_scan_tiles(long long* tsum, int ntiles, long long* total_out) {
    __shared__ long long s_w[16];
    const int t = (int)threadIdx.x;
    const int per = (ntiles + 1023) / 1024;                  // consecutive tiles of this thread
    const int a = min(t * per, ntiles), b = min(a + per, ntiles);
    long long s = 0;
    for (int k = a; k < b; ++k) s += tsum[k];
    long long total;
    long long run = nl_block_exclusive(s, s_w, total);
    for (int k = a; k < b; ++k) { const long long v = tsum[k]; tsum[k] = run; run += v; }
    if (t == 0) *total_out = total;
}

__global__ void __launch_bounds__(kNlScanThreads) k_nl_offsets(const int* __restrict__ counts, int n, const long long* __restrict__ tsum, long long* __restrict__ offsets) {
    __shared__ long long s_w[kNlScanThreads / 64];
    const int t = (int)threadIdx.x;
    const long long base = (long long)blockIdx.x * kNlScanTile + (long long)t * kNlScanItems;
    int c[kNlScanItems];
    long long s = 0;
#pragma unroll
    for (int e = 0; e < kNlScanItems; ++e) { c[e] = base + e < n ? counts[base + e] : 0; s += c[e]; }
    long long total;
    long long run = tsum[blockIdx.x] + nl_block_exclusive(s, s_w, total);
#pragma unroll
    for (int e = 0; e < kNlScanItems; ++e) { if (base + e < n) offsets[base + e] = run; run += c[e]; }
}

}  // namespace sphmi
