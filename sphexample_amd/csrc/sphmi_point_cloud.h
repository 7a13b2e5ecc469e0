// sphmi_point_cloud.h — pressure, density, velocity and fill sampled at ARBITRARY points, on demand (sphmi_sample_points).
//
// Per point the sums are the probes' and the lattice's (heads of sphmi_probes.h and sphmi_field_grid.h): over the rows j the handle
// owns with Type == Fluid and r² = ((dx² + dy²) + dz²) ≤ H² on the CURRENT positions, contraction off,
//     w_j = (m₀ / ρ_j) · W(r)      n = rows      S = Σ w_j      SP = Σ w_j P_j      Sρ = Σ w_j ρ_j      Sv = Σ w_j v_j
// on the state sphmi_download would deliver now.  No self term, r = 0 is legal, everything in fp64; the RAW sums are written, the
// host normalises (GridSums, sphmi_series.h).
//
// A probe is one wave that walks its ≤ 4^D cells alone; a lattice shares the staged rows among the 256 nodes of a brick because
// neighbouring nodes are neighbouring indices.  A cloud has no such order, so it is given one first.
//
// 1. BIN.  The dense cell grid (GridDesc) is tiled by BLOCKS of B cells per axis, B = pc_block_cells(dims).  A point takes the
//    block of the cell pc_plan_point gives it — the hash of the rows, trunc(|x|·H⁻¹ + ½) with the sign of x, in fp64 and not
//    fused, clamped per axis into the padded grid: a point outside the grid lands in the outermost block of that side.  The
//    block only GROUPS; no result depends on it (below), so the arithmetic need not be the handle's.
//        k_pc_count     one point per lane: its block → block_of[p], an integer atomic add to count[block]
//        k_pc_tiles     tcount[block] = pc_plan_tiles(count[block]) = ⌈count / 256⌉
//        scan64         (sphmi_results.h) of count → poff, of tcount → toff; toff[blocks] = the number of tiles, to the host
//        k_pc_scatter   slot = poff[block] + atomic add to cursor[block]; index[slot] = p
//        k_pc_describe  one lane per tile: the block b with toff[b] ≤ t < toff[b + 1] by a binary search, tile { first, count }
//    A TILE is at most 256 points of ONE block: slots [first, first + count) of `index`, which maps them back to the caller's
//    indices.  The atomics decide which slot, hence which lane of which tile of its block, a point lands in — nothing else.
//    B trades the candidate cells a tile stages against the lanes it fills: a tile's span is at most B cells plus the reach
//    cells per axis, (B + 4)^D cells at H = 2h, whatever the number of its points, while a cloud with fewer than 256 points per
//    occupied block leaves lanes idle.  B = 3 in 3-D (27 cells, 7³ candidates) and 6 in 2-D (36 cells, 10² candidates) fill a
//    tile from about eight points per cell upwards; the values are chosen by that arithmetic, not tuned by measurement.
//
// 2. SAMPLE.  k_point_cloud — one workgroup of four waves per tile, one point per lane; what k_field_grid does per brick:
//    * Candidate rows: per axis the span from the tile's smallest to its largest coordinate (a workgroup min / max), widened
//      by reach = H + h and the 1e-6 of the probes ("EXACT, NOT STALE", sphmi_probes.h) and clamped to the grid — the formulas
//      a brick applies to its first and last node.  Subtraction, multiplication by H⁻¹ > 0, ceil and floor are monotone, so
//      the span holds the candidate cells of the probe of every point of the tile.  Per (cy, cz) the x-adjacent cells are ONE
//      index range of `cstart`; the ranges are taken in (cz, cy, row) order, 256 per batch, and concatenated by a workgroup scan.
//    * Staging and walk: as in k_field_grid — chunks of 256 candidates, converted ONCE to { x, y, z, m₀/ρ, P, ρ, v } in fp64
//      in two LDS buffers, the next chunk's loads in flight while this one is walked; rows that are not Fluid, ghost copies and
//      dead rows are staged with x = NaN; every lane reads the staged rows as an LDS broadcast and applies the exact cut for
//      its own point.  Spare lanes of a tile carry a NaN position.
//    * WHAT A POINT'S RESULT DEPENDS ON: rows are sorted by cell, so (cz, cy, row) order is ascending row order.  A row the
//      tile stages beyond the point's own candidates fails the point's cut and adds nothing; the rows that pass are the rows
//      within H, added in ascending row order with one arithmetic, without atomics and without a cross-lane reduction.  The
//      bits therefore depend on the point's coordinates and the handle's state alone — not on the tile, the lane, the other
//      points of the call, their number or their order.  (tests/test_sample_points_gpu.py checks this bitwise.)
//    * Results go to the arena at the CALLER's index: seven arrays of n_points doubles { S, SP, Sρ, Sv[0..2], n }.
//    LDS and registers are k_field_grid's (four workgroups per compute unit, no scratch); the min / max borrows the first
//    staging buffer before the first chunk.
//
// COST.  A tile costs what a brick of the same span costs: the rows of at most (B + reach cells)^D cells staged once and walked
// by 256 lanes.  Only a cloud with fewer than 256 points per occupied block wastes lanes; its worst case, one point per block,
// is a span of the point's own ≤ 4^D (5^D for k < 2) cells — what a probe reads — walked by a workgroup of which one lane counts.
// A block with more than 256 points makes several tiles that each may span the whole block: their points are not sorted within it.
//
// The first part of this header is plain C++17 that also compiles as HIP (the plan: tests/host_points/points_main.cpp restates the
// bins of a cloud on a machine without a GPU); the kernels follow behind __HIPCC__.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "sphmi_series.h"       // kFgValues, kMaxSamplePoints

#ifndef SPHMI_HD
#if defined(__HIPCC__)
#define SPHMI_HD __host__ __device__ inline
#else
#define SPHMI_HD inline
#endif
#endif
#ifndef SPHMI_NO_CONTRACT
#if defined(__clang__)
#define SPHMI_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SPHMI_NO_CONTRACT                        /* (the host program is compiled with -ffp-contract=off) */
#endif
#endif

namespace sphmi {

constexpr int kPcTile = 256;                     // points of a tile: the lanes of a workgroup of k_point_cloud
constexpr int pc_block_cells(int dims) { return dims == 3 ? 3 : 6; }      // B (the head comment)

// the padded cell grid of the last rebuild (GridDesc) and its tiling by blocks; axes ≥ dims hold one cell and one block
struct PcTiling {
    int gmin[3], np[3], nb[3];
    int B, dims;
    double H_inv;
};
inline PcTiling pc_tiling(const int* gmin, const int* np, int dims, double H_inv) {
    PcTiling G{};
    G.B = pc_block_cells(dims); G.dims = dims; G.H_inv = H_inv;
    for (int d = 0; d < 3; ++d) {
        G.gmin[d] = d < dims ? gmin[d] : 0;
        G.np[d] = d < dims ? np[d] : 1;
        G.nb[d] = (G.np[d] + G.B - 1) / G.B;
    }
    return G;
}
SPHMI_HD long long pc_blocks(const PcTiling& G) { return (long long)G.nb[0] * G.nb[1] * G.nb[2]; }

// THE PLAN of a point: position → padded cell per axis (clamped into [0, np − 1]) → block per axis → block index, and of a block:
// points → tiles.  `x` holds `dims` finite doubles.
struct PcPlan { int cell[3]; int block; };
SPHMI_HD PcPlan pc_plan_point(const PcTiling& G, const double* x) {
    SPHMI_NO_CONTRACT
    PcPlan P{};
    int b[3] = {0, 0, 0};
    for (int d = 0; d < 3; ++d) {
        if (d >= G.dims) continue;
        const double t = trunc(fabs(x[d]) * G.H_inv + 0.5);
        const double c = x[d] < 0.0 ? -t : t;
        const double i = (c - (double)G.gmin[d]) + 1.0;                     // padded index 1 is cell gmin
        P.cell[d] = (int)fmin(fmax(i, 0.0), (double)(G.np[d] - 1));        // (in fp64 before the conversion: a point may be anywhere)
        b[d] = P.cell[d] / G.B;
    }
    P.block = b[0] + G.nb[0] * (b[1] + G.nb[1] * b[2]);
    return P;
}
SPHMI_HD int pc_plan_tiles(int count) { return (count + kPcTile - 1) / kPcTile; }

struct PcTile { int first, count; };             // slots [first, first + count) of the index array, 1 ≤ count ≤ kPcTile

}  // namespace sphmi

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "sphmi_kernels.h"
#include "sphmi_rebuild.h"
#include "sphmi_probes.h"       // pr_kernel_w
#include "sphmi_field_grid.h"   // kFgThreads, kFgRow, kFgLdsBytes

namespace sphmi {

static_assert(kPcTile == kFgThreads, "one point per lane");

__global__ void __launch_bounds__(256) k_pc_count(const double* pos, int n, const PcTiling G, int nblocks, int* block_of, int* count) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= n) return;
    double x[3] = {0.0, 0.0, 0.0};
    for (int d = 0; d < G.dims; ++d) x[d] = pos[(size_t)p * G.dims + d];
    const int b = min(max(pc_plan_point(G, x).block, 0), nblocks - 1);      // (the plan clamps; keeps every atomic inside the array)
    block_of[p] = b;
    atomicAdd(&count[b], 1);
}

__global__ void __launch_bounds__(256) k_pc_tiles(const int* count, int nblocks, int* tcount) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b < nblocks) tcount[b] = pc_plan_tiles(count[b]);
}

__global__ void __launch_bounds__(256) k_pc_scatter(const int* block_of, int n, const long long* poff, int* cursor, int* index) {
    const int p = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (p >= n) return;
    const int b = block_of[p];
    const long long slot = poff[b] + (long long)atomicAdd(&cursor[b], 1);
    if (slot >= 0 && slot < (long long)n) index[slot] = p;                  // (always, on a consistent count; keeps the store inside the array)
}

__global__ void __launch_bounds__(256) k_pc_describe(const long long* toff, const long long* poff, int nblocks, int ntiles, PcTile* tiles) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= ntiles) return;
    int a = 0, b = nblocks - 1;                                             // the last block with toff ≤ t: the one that holds tile t
    while (a < b) { const int m = (a + b + 1) >> 1; if (toff[m] <= (long long)t) a = m; else b = m - 1; }
    const int k = t - (int)toff[a];
    const long long c = poff[a + 1] - poff[a];
    PcTile T;
    T.first = (int)poff[a] + kPcTile * k;
    T.count = (int)min((long long)kPcTile, c - (long long)kPcTile * k);
    tiles[t] = T;
}

template <class T> struct PointCloudArgs {
    using V4 = typename Vec4<T>::type;
    Half<const V4> pk0, pk1;             // the set sphmi_download reads
    Half<const V4> half0;                // the half-step set: Pressure!(ρₙ⁺)
    const V4* comp;                      // fp32 handles: low words of position and density (null: none)
    const uint8_t* type;                 // slab handles: the type byte (ghost copies, dead rows); null on plain handles
    const int* cstart;
    const double* pos;                   // D doubles per point, the caller's order
    const PcTile* tiles;
    const int* index;                    // slot → the caller's index
    double* out;                         // kFgValues arrays of n_points doubles
    GridDesc g;
    long long n_points;
    double H_inv, H2, h_inv, reach;
    double alphaD, m0;
    T rho0, inv_rho0, Cbe;
    int N, kernel;
};

// The seven sums of a point, as one lane carries them through pc_walk.  `add` is handed one accepted row — the staged row r = { x, y, z,
// m₀/ρ, P, ρ, v }, its weight w, its distance and d = x_p − x_j — and `store` writes the slots 0 … 6 of every sampler of the family
// (M = n_points: the stride of a slot).  pc_walk is written over such a set; PcmSums (sphmi_point_moments.h) carries these seven,
// formed by these statements, and its own sums behind them.  A set also names what its kernel does for registers or speed and
// another does not (profiles/point_walk.md):
//     Count      the type the rows are counted in: a double here, an int where 24 more sums fill the registers of a lane
//     kUniform   the span of the tile and the chunk counts are declared uniform (readfirstlane): they and the loops over them live in
//                scalar registers.  The larger set needs it — its sums leave the vector file no room; here it is not set
//     kUnroll2   the row loop is unrolled by two; the larger set leaves its loop to the compiler
template <int D, class Count = double>
struct PcSums {
    static constexpr bool kUniform = false, kUnroll2 = true;
    Count n = 0;
    double S = 0.0, SP = 0.0, Sr = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0;
    template <class Args>
    __device__ __forceinline__ void add(const Args&, const double* r, double w, double, double, double, double) {
        const double rho = r[5];
        n += 1; S += w; SP += w * r[4]; Sr += w * rho;
        Sx += w * r[6]; Sy += w * r[7];
        if (D == 3) Sz += w * r[8];
    }
    __device__ __forceinline__ void store(double* o, long long M) const {
        o[0] = S; o[M] = SP; o[2 * M] = Sr; o[3 * M] = Sx; o[4 * M] = Sy; o[5 * M] = D == 3 ? Sz : 0.0;
        o[6 * M] = (double)n;
    }
};

// THE WALK of one workgroup over the candidate rows of its tile (SAMPLE in the head comment): from the point xp of this lane
// (has_point: the lane holds one; a spare lane's xp is set to NaN) to the sums of `s` (zero on entry) over the rows within H of xp, in
// ascending row order.  `Sums` names the per-row statements and the constants above.  k_point_cloud and k_point_moments call it
// and differ otherwise in their read of the point and their stores.  k_point_gradients (sphmi_point_gradients.h) keeps a COPY of
// this function in its body, because under the function it needs scratch (profiles/point_walk.md): a fix here has to be made
// there too.  The LDS — two staging buffers, the two range tables of a batch, four wave sums: 38 928 B — is k_field_grid's in
// every instantiation.
template <class T, int D, class Sums>
__device__ __forceinline__ void pc_walk(const PointCloudArgs<T>& A, double (&xp)[3], const bool has_point, Sums& s) {
    using V4 = typename Vec4<T>::type;
    constexpr bool kUniform = Sums::kUniform;
    auto uniform = [](int v) { return kUniform ? __builtin_amdgcn_readfirstlane(v) : v; };
    __shared__ double s_row[2][kFgThreads * kFgRow];
    __shared__ int s_rs[kFgThreads], s_incl[kFgThreads];
    __shared__ int s_wave[4];
    static_assert(sizeof(s_row) + sizeof(s_rs) + sizeof(s_incl) + sizeof(s_wave) <= kFgLdsBytes, "LDS of pc_walk: no more than k_field_grid");
    static_assert(4 * kFgLdsBytes <= 160 * 1024, "the LDS allows four workgroups per compute unit");
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;

    // the smallest and the largest coordinate of the tile per axis (count ≥ 1: both finite); the first staging buffer is free until the first chunk
    double mn[3] = {0.0, 0.0, 0.0}, mx[3] = {0.0, 0.0, 0.0};
    {
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            mn[d] = has_point ? xp[d] : inf; mx[d] = has_point ? xp[d] : -inf;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) { mn[d] = fmin(mn[d], __shfl_xor(mn[d], o, 64)); mx[d] = fmax(mx[d], __shfl_xor(mx[d], o, 64)); }
            if (lane == 0) { s_row[0][wave * 6 + d] = mn[d]; s_row[0][wave * 6 + 3 + d] = mx[d]; }
        }
        __syncthreads();
#pragma unroll
        for (int d = 0; d < D; ++d) {
            mn[d] = s_row[0][d]; mx[d] = s_row[0][3 + d];
#pragma unroll
            for (int w = 1; w < 4; ++w) { mn[d] = fmin(mn[d], s_row[0][w * 6 + d]); mx[d] = fmax(mx[d], s_row[0][w * 6 + 3 + d]); }
        }
        __syncthreads();
    }
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool empty = false;
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (d >= D) continue;
            // the span of the tile, padded and clamped like a probe's and a brick's
            double a = (mn[d] - A.reach) * A.H_inv, b = (mx[d] + A.reach) * A.H_inv;
            a -= 1e-6 * (1.0 + fabs(a)); b += 1e-6 * (1.0 + fabs(b));
            const double off = 1.0 - (double)A.g.gmin[d], top = (double)(A.g.np[d] - 1);
            const double l = fmax(ceil(a - 0.5) + off, 0.0), u = fmin(floor(b + 0.5) + off, top);
            if (!(l <= u) || a != a || b != b) empty = true;        // outside the grid (NaN: ∞ − ∞ of a coordinate beyond 1e308·H, which nothing is near)
            lo[d] = empty ? 0 : (int)l; hi[d] = empty ? 0 : (int)u;
        }
    }
    if (!has_point) xp[0] = __longlong_as_double(0x7ff8000000000000ll);      // fails every cut
    // (every lane holds the same span — it comes from the workgroup's min / max; kUniform says so)
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo[d] = uniform(lo[d]); hi[d] = uniform(hi[d]); }
    const int ny = hi[1] - lo[1] + 1, nz = D == 3 ? hi[2] - lo[2] + 1 : 1;
    const int nrange = uniform((int)empty) ? 0 : ny * nz;

    for (int rbase = 0; rbase < nrange; rbase += kFgThreads) {
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
        const int total = uniform(s_incl[kFgThreads - 1]);
        const int nchunk = (total + kFgThreads - 1) / kFgThreads;

        V4 q0, q1, lw;
        T hw = T(0);
        uint8_t ty = 0;
        bool ok = false;
        auto load = [&](int c) {
            const int q = c * kFgThreads + t;
            ok = q < total;
            int k = 0;
            if (ok) {
                int a = 0, b = kFgThreads - 1;               // the first range with s_incl > q
                while (a < b) { const int m = (a + b) >> 1; if (s_incl[m] > q) b = m; else a = m + 1; }
                k = s_rs[a] + q;
            }
            q0 = A.pk0[k]; q1 = A.pk1[k]; hw = A.half0[k].w;
            if (sizeof(T) == 4 && A.comp) lw = A.comp[k]; else { lw.x = lw.y = lw.z = lw.w = T(0); }
            ty = A.type ? A.type[k] : (uint8_t)(q0.w > T(0) ? 1 : 2);
        };
        auto stage = [&](int buf) {
            double* r = &s_row[buf][t * kFgRow];
            const bool fluid = ok && (ty & kTypeMask) == 1 && !(ty & kGhostMask);      // SPHMI_FLUID, owned
            const double rho = (double)(q0.w < T(0) ? -q0.w : q0.w) + (double)lw.w;
            // Pressure as k_pack_output delivers it: Pressure!(ρₙ⁺) in the handle's arithmetic
            const T rr = sizeof(T) == 8 ? hw / A.rho0 : hw * A.inv_rho0;
            const T rr2 = rr * rr, rr4 = rr2 * rr2;
            r[0] = fluid ? (double)q0.x + (double)lw.x : __longlong_as_double(0x7ff8000000000000ll);
            r[1] = (double)q0.y + (double)lw.y;
            r[2] = (double)q0.z + (double)lw.z;
            r[3] = A.m0 / rho;
            r[4] = (double)(A.Cbe * (rr4 * rr2 * rr - T(1)));
            r[5] = rho;
            r[6] = (double)q1.x; r[7] = (double)q1.y; r[8] = (double)q1.z;
        };
        auto row = [&](const double* r) {
            double dx, dy, dz, r2;
            {
                // (no contraction: r² is ((dx² + dy²) + dz²) rounded term by term, as in k_probe_sample and k_field_grid)
#pragma clang fp contract(off)
                dx = xp[0] - r[0]; dy = xp[1] - r[1]; dz = D == 3 ? xp[2] - r[2] : 0.0;
                r2 = dx * dx + dy * dy + dz * dz;
            }
            if (r2 <= A.H2) {
                const double dist = sqrt(r2);
                s.add(A, r, r[3] * pr_kernel_w(A.kernel, A.alphaD, dist * A.h_inv), dist, dx, dy, dz);
            }
        };
        if (nchunk > 0) { load(0); stage(0); }
        __syncthreads();
        for (int c = 0; c < nchunk; ++c) {
            const bool more = c + 1 < nchunk;
            if (more) load(c + 1);                           // in flight while chunk c is walked
            const double* R = s_row[c & 1];
            const int cnt = min(kFgThreads, total - c * kFgThreads);
            if (Sums::kUnroll2) {
#pragma unroll 2
                for (int j = 0; j < cnt; ++j) row(R + j * kFgRow);
            } else {
                for (int j = 0; j < cnt; ++j) row(R + j * kFgRow);
            }
            if (more) stage((c + 1) & 1);                    // the buffer chunk c − 1 was walked from: every lane is past the barrier behind it
            __syncthreads();
        }
    }
}

template <class T, int D>
__global__ void __launch_bounds__(kFgThreads, 4) k_point_cloud(const PointCloudArgs<T> A) {
    const int t = (int)threadIdx.x;
    // the tile of this workgroup, the point of this lane
    const PcTile tile = A.tiles[blockIdx.x];
    const bool has_point = t < tile.count;
    long long p = 0;
    double xp[3] = {0.0, 0.0, 0.0};
    if (has_point) {
        p = (long long)A.index[tile.first + t];
        if (p < 0 || p >= A.n_points) p = 0;                 // (cannot happen on a consistent index; keeps every access inside the arrays)
#pragma unroll
        for (int d = 0; d < D; ++d) xp[d] = A.pos[p * D + d];
    }
    PcSums<D> s;
    pc_walk<T, D>(A, xp, has_point, s);
    if (has_point) s.store(A.out + p, A.n_points);
}

}  // namespace sphmi
#endif  // __HIPCC__
