// sphmi_point_moments.h — the MOMENT sums of the kernel weights at arbitrary points, on demand (sphmi_sample_point_moments): what a
// first-order moving-least-squares fit needs — the linear reconstruction mDBC makes at its ghost nodes (k_mdbc), offered at any cloud
// of points — and, every sum being linear in the rows, on multi-device handles too.
//
// Per point x, over the rows j the handle owns with Type == Fluid and r² = ((dx² + dy²) + dz²) ≤ H² on the CURRENT positions,
// contraction off (the cut of k_point_cloud), with w_j = (m₀ / ρ_j) W(r) and e_j = x_j − x:
//     n = rows      S = Σ w      SP = Σ w P      Sρ = Σ w ρ      Sv[a] = Σ w v[a]
//     M1[b] = Σ w e[b]      M2[bc] = Σ w e[b] e[c]  (xx, xy, xz, yy, yz, zz)
//     P1[b] = Σ w P e[b]    R1[b] = Σ w ρ e[b]      V1[a][b] = Σ w v[a] e[b]
// on the state sphmi_download would deliver now (record + low word on fp32 handles, Pressure!(ρₙ⁺) of the half-step set), all in
// fp64, no self term.  A row at r = 0 counts in n and the zeroth sums and adds nothing to the others (e = 0).  The RAW sums are
// written and delivered; the caller solves [[S, M1ᵀ], [M1, M2]] · [a; b] = [Σ w f; Σ w f e] per point and field
// (sphexample_amd/fields.py: linear_fit), which is exact for a linear field however one-sided the support.
//
// k_point_moments — the walk of k_point_gradients (sphmi_point_gradients.h) with other sums and without pf_kernel.  The cloud is
// binned by the BIN passes of sphmi_point_cloud.h, as they are; one workgroup of four waves per tile, one point per lane; the
// candidate span, the range scan, the chunks of 256 rows staged once in fp64 in two LDS buffers, the walk as an LDS broadcast with
// the exact cut per lane: all as there.  n, S, SP, Sρ and Sv are formed by the statements of k_point_cloud, so that they are the
// sums sphmi_sample_points and sphmi_sample_point_gradients deliver, bit for bit.  Rows are added in ascending row order, without
// atomics and without a cross-lane reduction: a point's bits depend on its coordinates and the handle's state alone.
//
// Budget, read off the code object by tests/test_point_moments_host.py: the LDS is k_point_cloud's (38 928 B).  In 3-D a lane carries
// 30 fp64 sums and the row count — six more than k_point_gradients, which fills the 128 registers that four waves per SIMD leave a
// lane — so the kernel is declared for two workgroups per compute unit (256 registers) and takes what it needs without scratch:
// 128 registers with fp32 records (no pf_kernel: it still runs at four workgroups per compute unit), 134 with fp64 records (three),
// 100 / 104 in 2-D.  The alternative — two launches of 18 and 12 sums, each within 128 registers at four workgroups — walks the rows
// twice and measured 6.2 ms against 3.5 ms for this one kernel on the bench case (profiles/point_moments.md).
//
// Results go to the arena at the CALLER's index: kPmValues arrays of n_points doubles — slots 0 … 6 are k_point_cloud's
// { S, SP, Sρ, Sv[0..2], n }, then M1 at 7, M2 at 10, P1 at 16, R1 at 19 and V1[a][b] at 22 + 3a + b.  2-D handles write exact zeros
// to every slot of the third axis.  The host reads this layout from ONE table, kPmOutputs (sphmi_series.h): which slots an output
// needs and where they go; the stores at the end of the kernel assert the slots they fill.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_point_cloud.h"       // PcTile, PointCloudArgs, the BIN passes; kFgThreads, kFgRow, kFgLdsBytes, pr_kernel_w

namespace sphmi {

static_assert(kPmValues == kFgValues + 24, "the sums of k_point_cloud, then M1, M2, P1, R1 and V1");

// the arguments are k_point_cloud's; `out` holds kPmValues arrays of n_points doubles
template <class T, int D>
__global__ void __launch_bounds__(kFgThreads, 2) k_point_moments(const PointCloudArgs<T> A) {
    using V4 = typename Vec4<T>::type;
    __shared__ double s_row[2][kFgThreads * kFgRow];
    __shared__ int s_rs[kFgThreads], s_incl[kFgThreads];
    __shared__ int s_wave[4];
    static_assert(sizeof(s_row) + sizeof(s_rs) + sizeof(s_incl) + sizeof(s_wave) <= kFgLdsBytes, "LDS of k_point_moments: no more than k_field_grid");
    static_assert(4 * kFgLdsBytes <= 160 * 1024, "the LDS allows four workgroups of k_point_moments per compute unit");
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;

    // the tile of this workgroup, the point of this lane
    const PcTile tile = A.tiles[blockIdx.x];
    const bool has_point = t < tile.count;
    // (the caller's index of the point is read here and AGAIN before the stores, as in k_point_gradients: it is not carried through the walk)
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
    // over them live in scalar registers
#pragma unroll
    for (int d = 0; d < 3; ++d) { lo[d] = __builtin_amdgcn_readfirstlane(lo[d]); hi[d] = __builtin_amdgcn_readfirstlane(hi[d]); }
    const int ny = hi[1] - lo[1] + 1, nz = D == 3 ? hi[2] - lo[2] + 1 : 1;
    const int nrange = __builtin_amdgcn_readfirstlane((int)empty) ? 0 : ny * nz;

    int n = 0;
    double S = 0.0, SP = 0.0, Sr = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0;
    double M1[3] = {0.0, 0.0, 0.0}, P1[3] = {0.0, 0.0, 0.0}, R1[3] = {0.0, 0.0, 0.0};
    double M2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double V1[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
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
                    const double dist = sqrt(r2);
                    const double w = r[3] * pr_kernel_w(A.kernel, A.alphaD, dist * A.h_inv);
                    // w e with e = x_j − x = −(dx, dy, dz): every moment is one product with it
                    const double wx = w * -dx, wy = w * -dy, wz = w * -dz;
                    const double rho = r[5];
                    n += 1; S += w; SP += w * r[4]; Sr += w * rho;
                    Sx += w * r[6]; Sy += w * r[7];
                    M1[0] += wx; M1[1] += wy;
                    M2[0] += wx * -dx; M2[1] += wx * -dy; M2[3] += wy * -dy;
                    P1[0] += r[4] * wx; P1[1] += r[4] * wy;
                    R1[0] += rho * wx; R1[1] += rho * wy;
                    V1[0][0] += r[6] * wx; V1[0][1] += r[6] * wy;
                    V1[1][0] += r[7] * wx; V1[1][1] += r[7] * wy;
                    if (D == 3) {
                        Sz += w * r[8];
                        M1[2] += wz;
                        M2[2] += wx * -dz; M2[4] += wy * -dz; M2[5] += wz * -dz;
                        P1[2] += r[4] * wz; R1[2] += rho * wz;
                        V1[0][2] += r[6] * wz; V1[1][2] += r[7] * wz;
                        V1[2][0] += r[8] * wx; V1[2][1] += r[8] * wy; V1[2][2] += r[8] * wz;
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
        // the slots below are the entries moment1, moment2, moment_pressure, moment_density and moment_velocity of kPmOutputs
        static_assert(kPmOutputs[3].first == 7 && kPmOutputs[4].first == 10 && kPmOutputs[5].first == 16 && kPmOutputs[6].first == 19 && kPmOutputs[7].first == 22,
                      "the stores of k_point_moments fill the slots of kPmOutputs");
        // (xx, xy, xz, yy, yz, zz: the entries with a z index are 2, 4 and 5)
        o[10 * M] = M2[0]; o[11 * M] = M2[1]; o[12 * M] = D == 3 ? M2[2] : 0.0;
        o[13 * M] = M2[3]; o[14 * M] = D == 3 ? M2[4] : 0.0; o[15 * M] = D == 3 ? M2[5] : 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const bool z = b >= D;                           // a slot of the third axis on a 2-D handle: an exact zero
            o[(7 + b) * M] = z ? 0.0 : M1[b];
            o[(16 + b) * M] = z ? 0.0 : P1[b];
            o[(19 + b) * M] = z ? 0.0 : R1[b];
#pragma unroll
            for (int a = 0; a < 3; ++a) o[(22 + 3 * a + b) * M] = (z || a >= D) ? 0.0 : V1[a][b];
        }
    }
}

}  // namespace sphmi
