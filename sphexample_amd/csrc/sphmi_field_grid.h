// sphmi_field_grid.h — pressure, density, velocity and fill sampled on a regular lattice, on demand (sphmi_sample_grid).
//
// Per lattice node the sums are the probes' (head of sphmi_probes.h): over the rows j the handle owns with Type == Fluid and
// |x_n − x_j|² ≤ H² on the CURRENT positions,
//     w_j = (m₀ / ρ_j) · W(|x_n − x_j|)      n = rows      S = Σ w_j      SP = Σ w_j P_j      Sρ = Σ w_j ρ_j      Sv = Σ w_j v_j
// on the state sphmi_download would deliver now: Position and Density record + low word on fp32 handles, Velocity of the
// current set, Pressure = Pressure!(ρₙ⁺) of the half-step set in the handle's arithmetic.  No self term, r = 0 is legal, r² is
// ((dx² + dy²) + dz²) with contraction off — the value k_probe_sample and a host reference form: a row AT the cut is in or
// out for all three.  Everything is summed in fp64; the RAW sums are written, the host normalises.
//
// k_field_grid — where a probe is one wave that walks its ≤ 4^D cells alone, a lattice shares them.  The lattice is cut into
// BRICKS of bx × by × bz ≤ 256 nodes (fg_plan_brick, on the host); one workgroup of four waves takes a brick, one node per
// lane.  Node (i, j, k) lies at origin[d] + (double)i_d · spacing[d], one multiply and one add, not fused.
//   * Candidate rows: the cells of the brick's first and last node, widened per axis by reach = H + h and the 1e-6 the
//     probes derive ("EXACT, NOT STALE", sphmi_probes.h) — by monotony of ceil / floor this span holds the candidate cells
//     of every node of the brick, so every node sees exactly the rows its own probe would.  Per (cy, cz) the x-adjacent
//     cells are ONE index range of `cstart`; the ranges are taken in (cz, cy, row) order, 256 of them per batch, and
//     concatenated by a workgroup scan into one dense stream of candidates.
//   * Staging: the stream is cut into chunks of 256 candidates.  Lane t finds candidate 256·c + t by a binary search of
//     the scan (eight LDS reads), loads its row — both packets, the half-step density, fp32: the low words; consecutive
//     lanes read consecutive rows of a range — and converts it ONCE to { x, y, z, m₀/ρ, P, ρ, v } in fp64.  A row that is
//     not Fluid, a ghost copy or dead is staged with x = NaN: it fails every cut.  Two buffers: the loads of chunk c + 1
//     are issued before chunk c is walked and written behind the walk, one barrier per chunk.
//   * Walk: every lane reads the staged rows in order — all lanes the same LDS address, a broadcast — applies the exact cut
//     for its own node and accumulates.  The fp64 conversion, the EOS and m₀/ρ are paid once per row and brick, not once
//     per row and node.
// The order of every sum is the row order (cz, cy, row): no atomics, no cross-lane reduction, the same bits on every call.
// A brick whose ranges are all empty — most of a tank-sized lattice is air — writes zeros after one batch of `cstart`
// reads; a node outside the dense grid clamps to empty ranges like a probe.  Lanes of a brick that hang over the lattice
// carry a NaN position.
//
// Results: seven arrays of `nodes` doubles { S, SP, Sρ, Sv[0..2], n } in the handle's arena, node index i + nx·(j + ny·k);
// a lane's bx neighbours along x store side by side.  2-D handles write a zero third velocity component.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_kernels.h"
#include "sphmi_rebuild.h"
#include "sphmi_probes.h"
#include "sphmi_series.h"       // kFgValues, kMaxGridNodes

namespace sphmi {

constexpr int kFgThreads = 256;                  // nodes of a brick, candidates of a chunk, ranges of a batch
constexpr int kFgRow = 9;                        // doubles of a staged row: x, y, z, m₀/ρ, P, ρ, v[3]
constexpr size_t kFgLdsBytes = 2 * (size_t)kFgThreads * kFgRow * 8 + 2 * (size_t)kFgThreads * 4 + 64;

template <class T> struct FieldGridArgs {
    using V4 = typename Vec4<T>::type;
    Half<const V4> pk0, pk1;             // the set sphmi_download reads
    Half<const V4> half0;                // the half-step set: Pressure!(ρₙ⁺)
    const V4* comp;                      // fp32 handles: low words of position and density (null: none)
    const uint8_t* type;                 // slab handles: the type byte (ghost copies, dead rows); null on plain handles
    const int* cstart;
    double* out;                         // kFgValues arrays of `nodes` doubles
    GridDesc g;
    double origin[3], spacing[3];
    long long nodes;
    int counts[3], brick[3], nbricks[3];
    double H_inv, H2, h_inv, reach;
    double alphaD, m0;
    T rho0, inv_rho0, Cbe;
    int N, kernel;
};

// The nodes of a brick per axis: as many as fit into 256, grown one at a time along the axis on which the brick is
// shortest — the candidate span of a brick is (extent + 2·reach) per axis, and for a fixed number of nodes the product is
// smallest for a cube.  (Wave time is what a brick costs, whatever the number of its lanes that carry a node: fewer
// than 256 nodes per brick is never cheaper per node.)
inline void fg_plan_brick(int D, const double* spacing, const int64_t* counts, int brick[3]) {
    brick[0] = brick[1] = brick[2] = 1;
    for (;;) {
        int best = -1;
        for (int d = 0; d < D; ++d) {
            if (brick[d] >= counts[d]) continue;
            if ((long long)brick[0] * brick[1] * brick[2] / brick[d] * (brick[d] + 1) > kFgThreads) continue;
            if (best < 0 || brick[d] * spacing[d] < brick[best] * spacing[best]) best = d;
        }
        if (best < 0) return;
        brick[best] += 1;
    }
}

template <class T, int D>
__global__ void __launch_bounds__(kFgThreads, 4) k_field_grid(const FieldGridArgs<T> A) {
    using V4 = typename Vec4<T>::type;
    __shared__ double s_row[2][kFgThreads * kFgRow];
    __shared__ int s_rs[kFgThreads], s_incl[kFgThreads];
    __shared__ int s_wave[4];
    static_assert(sizeof(s_row) + sizeof(s_rs) + sizeof(s_incl) + sizeof(s_wave) <= kFgLdsBytes, "LDS of k_field_grid");
    static_assert(4 * kFgLdsBytes <= 160 * 1024, "four workgroups of k_field_grid per compute unit");
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;

    // the brick of this workgroup, its first and last node per axis, the node of this lane
    int first[3] = {0, 0, 0}, last[3] = {0, 0, 0}, mine[3] = {0, 0, 0};
    {
        long long b = (long long)blockIdx.x;
        const int bi = (int)(b % A.nbricks[0]); b /= A.nbricks[0];
        const int bj = (int)(b % A.nbricks[1]), bk = (int)(b / A.nbricks[1]);
        const int bc[3] = {bi, bj, bk};
#pragma unroll
        for (int d = 0; d < 3; ++d) { first[d] = bc[d] * A.brick[d]; last[d] = min(first[d] + A.brick[d], A.counts[d]) - 1; }
        mine[0] = first[0] + t % A.brick[0];
        mine[1] = first[1] + (t / A.brick[0]) % A.brick[1];
        mine[2] = first[2] + t / (A.brick[0] * A.brick[1]);
    }
    const bool has_node = mine[0] <= last[0] && mine[1] <= last[1] && mine[2] <= last[2];
    double xp[3] = {0.0, 0.0, 0.0};
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool empty = false;
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (d >= D) continue;
            const double step = (double)mine[d] * A.spacing[d];
            xp[d] = A.origin[d] + step;
            // the span of the brick (spacing > 0: the first node is the lowest, the last the highest), padded and clamped like a probe's
            const double sf = (double)first[d] * A.spacing[d], sl = (double)last[d] * A.spacing[d];
            const double xf = A.origin[d] + sf, xl = A.origin[d] + sl;
            double a = (xf - A.reach) * A.H_inv, b = (xl + A.reach) * A.H_inv;
            a -= 1e-6 * (1.0 + fabs(a)); b += 1e-6 * (1.0 + fabs(b));
            const double off = 1.0 - (double)A.g.gmin[d], top = (double)(A.g.np[d] - 1);
            const double l = fmax(ceil(a - 0.5) + off, 0.0), u = fmin(floor(b + 0.5) + off, top);
            if (!(l <= u)) empty = true;
            lo[d] = empty ? 0 : (int)l; hi[d] = empty ? 0 : (int)u;
        }
    }
    if (!has_node) xp[0] = __longlong_as_double(0x7ff8000000000000ll);      // fails every cut
    const int ny = hi[1] - lo[1] + 1, nz = D == 3 ? hi[2] - lo[2] + 1 : 1;
    const int nrange = empty ? 0 : ny * nz;

    double n = 0.0, S = 0.0, SP = 0.0, Sr = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0;
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
        const int total = s_incl[kFgThreads - 1];
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
        if (nchunk > 0) { load(0); stage(0); }
        __syncthreads();
        for (int c = 0; c < nchunk; ++c) {
            const bool more = c + 1 < nchunk;
            if (more) load(c + 1);                           // in flight while chunk c is walked
            const double* R = s_row[c & 1];
            const int cnt = min(kFgThreads, total - c * kFgThreads);
#pragma unroll 2
            for (int j = 0; j < cnt; ++j) {
                const double* r = R + j * kFgRow;
                double r2;
                {
                    // (no contraction: r² is ((dx² + dy²) + dz²) rounded term by term, as in k_probe_sample)
#pragma clang fp contract(off)
                    const double dx = xp[0] - r[0], dy = xp[1] - r[1], dz = D == 3 ? xp[2] - r[2] : 0.0;
                    r2 = dx * dx + dy * dy + dz * dz;
                }
                if (r2 <= A.H2) {
                    const double rho = r[5];
                    const double w = r[3] * pr_kernel_w(A.kernel, A.alphaD, sqrt(r2) * A.h_inv);
                    n += 1.0; S += w; SP += w * r[4]; Sr += w * rho;
                    Sx += w * r[6]; Sy += w * r[7];
                    if (D == 3) Sz += w * r[8];
                }
            }
            if (more) stage((c + 1) & 1);                    // the buffer chunk c − 1 was walked from: every lane is past the barrier behind it
            __syncthreads();
        }
    }
    if (has_node) {
        const long long at = (long long)mine[0] + (long long)A.counts[0] * ((long long)mine[1] + (long long)A.counts[1] * (long long)mine[2]);
        double* o = A.out + at;
        o[0] = S; o[A.nodes] = SP; o[2 * A.nodes] = Sr; o[3 * A.nodes] = Sx; o[4 * A.nodes] = Sy; o[5 * A.nodes] = D == 3 ? Sz : 0.0;
        o[6 * A.nodes] = n;
    }
}

}  // namespace sphmi
