// sphmi_point_gradients.h — the GRADIENTS of pressure, density, velocity and fill at arbitrary points, on demand
// (sphmi_sample_point_gradients): what sphmi_particle_fields forms at the particles, at any cloud of points instead, and — every sum
// being linear in the rows — on multi-device handles too.
//
// Per point x, over the rows j the handle owns with Type == Fluid and r² = ((dx² + dy²) + dz²) ≤ H² on the CURRENT positions,
// contraction off (the cut of k_point_cloud), with V_j = m₀ / ρ_j, W and W′ the handle's kernel and g_j = W′(r) · (x − x_j) / r:
//     n = rows      S = Σ V_j W      SP = Σ V_j P_j W      Sρ = Σ V_j ρ_j W      Sv[a] = Σ V_j v_j[a] W
//     G[b] = Σ V_j g_j[b]      GP[b] = Σ V_j P_j g_j[b]      Gρ[b] = Σ V_j ρ_j g_j[b]      Gv[a][b] = Σ V_j v_j[a] g_j[b]
// on the state sphmi_download would deliver now (record + low word on fp32 handles, Pressure!(ρₙ⁺) of the half-step set), all in
// fp64, no self term.  A row at r = 0 counts in n and the S sums and adds nothing to the G sums: W′ / r is finite there (pf_kernel)
// and multiplies x − x_j = 0.  The RAW sums are written and delivered; the caller normalises (sphexample_amd/fields.py: the
// Shepard-corrected difference form ∇A ≈ (GA − (SA / S) · G) / S).
//
// k_point_gradients — k_point_cloud (sphmi_point_cloud.h) with more sums per row.  The body below is the one remaining COPY of
// pc_walk (there: the walk under k_point_cloud and k_point_moments): under the function this kernel's <double, 3> instantiation, which
// fills its 128 registers, needs 12 bytes of scratch (profiles/point_walk.md).  A fix to the span, the staging or the cut there has to
// be made here too, and the other way round.  The cloud is binned by the BIN passes of that
// header, as they are (k_pc_count, k_pc_tiles, scan64 twice, k_pc_scatter, k_pc_describe: tiles of at most 256 points of one block
// of cells); one workgroup of four waves per tile, one point per lane; the candidate span from the tile's min / max coordinates, the
// range scan, the chunks of 256 rows converted once to { x, y, z, V, P, ρ, v } in fp64 (kFgRow doubles; rows that are not Fluid,
// ghost copies and dead rows with x = NaN), two LDS buffers, the walk as an LDS broadcast with the exact cut per lane: all as there.
// n, S, SP, Sρ and Sv are formed by the statements of k_point_cloud — w = V · pr_kernel_w(q), then S += w, SP += w · P … — so that
// they are the sums sphmi_sample_points delivers; the G sums use W′ / r of pf_kernel (sphmi_particle_fields.h) on the same r.
// Rows are added in ascending row order, without atomics and without a cross-lane reduction: a point's bits depend on its
// coordinates and the handle's state alone, not on its tile, its lane or the other points of the call.
//
// Results go to the arena at the CALLER's index: kPgValues arrays of n_points doubles — slots 0 … 6 are k_point_cloud's
// { S, SP, Sρ, Sv[0..2], n }, then G[0..2], GP[0..2], Gρ[0..2] and Gv[a][b] at 16 + 3a + b.  2-D handles write exact zeros to
// every z slot (Sv[2], G[2], GP[2], Gρ[2], Gv[2][·], Gv[·][2]).  The host reads this layout from ONE table, kPgOutputs
// (sphmi_series.h): which slots an output needs and where they go; the stores at the end of the kernel assert the slots they fill.
//
// Budget, read off the code object by tests/test_point_gradients_host.py: the LDS is k_point_cloud's (38 928 B: four workgroups per
// compute unit); in 3-D a lane carries 24 fp64 sums and the row count, and the kernel takes 128 (fp64 records) / 126 (fp32) of the
// 128 registers that four waves per SIMD leave a lane, 110 / 106 in 2-D — no scratch, occupancy as the sibling kernels.  It fits
// because the tile's span, the chunk counts and the loops over them are declared uniform (readfirstlane: scalar registers) and
// the caller's index of a point is read again before the stores instead of being carried through the walk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_point_cloud.h"       // PcTile, PointCloudArgs, the BIN passes; kFgThreads, kFgRow, kFgLdsBytes, pr_kernel_w
#include "sphmi_particle_fields.h"   // pf_kernel

namespace sphmi {

static_assert(kPgValues == kFgValues + 18, "the sums of k_point_cloud, then G, GP, Gρ and Gv");

// the arguments are k_point_cloud's; `out` holds kPgValues arrays of n_points doubles
template <class T, int D>
__global__ void __launch_bounds__(kFgThreads, 4) k_point_gradients(const PointCloudArgs<T> A) {
    using V4 = typename Vec4<T>::type;
    __shared__ double s_row[2][kFgThreads * kFgRow];
    __shared__ int s_rs[kFgThreads], s_incl[kFgThreads];
    __shared__ int s_wave[4];
    static_assert(sizeof(s_row) + sizeof(s_rs) + sizeof(s_incl) + sizeof(s_wave) <= kFgLdsBytes, "LDS of k_point_gradients: no more than k_field_grid");
    static_assert(4 * kFgLdsBytes <= 160 * 1024, "four workgroups of k_point_gradients per compute unit");
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;

    // the tile of this workgroup, the point of this lane
    const PcTile tile = A.tiles[blockIdx.x];
    const bool has_point = t < tile.count;
    // (the caller's index of the point is read here and AGAIN before the stores, and the rows are counted in an int: the 25 sums
    // of the 3-D kernel fill the 128 registers of a lane, and neither value is carried through the walk.  The empty asm keeps the
    // compiler from merging the two reads, which would carry the 64-bit slot instead.)
    auto caller_index = [&]() {
        int slot = tile.first + t;
        asm volatile("" : "+v"(slot));
        const long long q = (long long)A.index[slot];
        return (q < 0 || q >= A.n_points) ? 0ll : q;         // (cannot happen on a consistent index; keeps every access inside the arrays)
    };
    double xp[3] = {0.0, 0.0, 0.0};
    if (has_point) {
        const long long p = caller_index();
#pragma unroll
        for (int d = 0; d < D; ++d) xp[d] = A.pos[p * D + d];
    }
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
    // every lane holds the same span (it comes from the workgroup's min / max): say so, and the span, the chunk counts and the loops
    // over them live in scalar registers — the 25 sums of a lane leave the vector file no room for them
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo[d] = __builtin_amdgcn_readfirstlane(lo[d]); hi[d] = __builtin_amdgcn_readfirstlane(hi[d]); }
    const int ny = hi[1] - lo[1] + 1, nz = D == 3 ? hi[2] - lo[2] + 1 : 1;
    const int nrange = __builtin_amdgcn_readfirstlane((int)empty) ? 0 : ny * nz;

    int n = 0;
    double S = 0.0, SP = 0.0, Sr = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0;
    double G[3] = {0.0, 0.0, 0.0}, GP[3] = {0.0, 0.0, 0.0}, Gr[3] = {0.0, 0.0, 0.0};
    double Gv[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
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
        const int total = __builtin_amdgcn_readfirstlane(s_incl[kFgThreads - 1]);
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
            for (int j = 0; j < cnt; ++j) {
                const double* r = R + j * kFgRow;
                double dx, dy, dz, r2;
                {
                    // (no contraction: r² is ((dx² + dy²) + dz²) rounded term by term, as in k_probe_sample and k_point_cloud)
#pragma clang fp contract(off)
                    dx = xp[0] - r[0]; dy = xp[1] - r[1]; dz = D == 3 ? xp[2] - r[2] : 0.0;
                    r2 = dx * dx + dy * dy + dz * dz;
                }
                if (r2 <= A.H2) {
                    const double rho = r[5];
                    const double dist = sqrt(r2);
                    const double w = r[3] * pr_kernel_w(A.kernel, A.alphaD, dist * A.h_inv);
                    n += 1; S += w; SP += w * r[4]; Sr += w * rho;
                    Sx += w * r[6]; Sy += w * r[7];
                    if (D == 3) Sz += w * r[8];
                    // V_j g_j = V_j (W′ / r) · (dx, dy, dz): zero at r = 0; every G sum is one product with it
                    double W, F;
                    pf_kernel(A.kernel, A.alphaD, A.h_inv, dist, W, F);
                    F *= r[3];
                    const double gx = F * dx, gy = F * dy;
                    G[0] += gx; G[1] += gy;
                    GP[0] += r[4] * gx; GP[1] += r[4] * gy;
                    Gr[0] += rho * gx; Gr[1] += rho * gy;
                    Gv[0][0] += r[6] * gx; Gv[0][1] += r[6] * gy;
                    Gv[1][0] += r[7] * gx; Gv[1][1] += r[7] * gy;
                    if (D == 3) {
                        const double gz = F * dz;
                        G[2] += gz; GP[2] += r[4] * gz; Gr[2] += rho * gz;
                        Gv[0][2] += r[6] * gz; Gv[1][2] += r[7] * gz;
                        Gv[2][0] += r[8] * gx; Gv[2][1] += r[8] * gy; Gv[2][2] += r[8] * gz;
                    }
                }
            }
            if (more) stage((c + 1) & 1);                    // the buffer chunk c − 1 was walked from: every lane is past the barrier behind it
            __syncthreads();
        }
    }
    if (has_point) {
        double* o = A.out + caller_index();
        const long long M = A.n_points;
        o[0] = S; o[M] = SP; o[2 * M] = Sr; o[3 * M] = Sx; o[4 * M] = Sy; o[5 * M] = D == 3 ? Sz : 0.0;
        o[6 * M] = (double)n;
        // the slots below are the entries grad_weight, grad_pressure, grad_density and grad_velocity of kPgOutputs
        static_assert(kPgOutputs[3].first == 7 && kPgOutputs[4].first == 10 && kPgOutputs[5].first == 13 && kPgOutputs[6].first == 16, "the stores of k_point_gradients fill the slots of kPgOutputs");
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const bool z = b >= D;                           // a slot of the third axis on a 2-D handle: an exact zero
            o[(7 + b) * M] = z ? 0.0 : G[b];
            o[(10 + b) * M] = z ? 0.0 : GP[b];
            o[(13 + b) * M] = z ? 0.0 : Gr[b];
#pragma unroll
            for (int a = 0; a < 3; ++a) o[(16 + 3 * a + b) * M] = (z || a >= D) ? 0.0 : Gv[a][b];
        }
    }
}

}  // namespace sphmi
