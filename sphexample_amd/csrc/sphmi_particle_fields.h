// sphmi_particle_fields.h — vorticity, velocity divergence, the free-surface indicator ∇·r, the free-surface normal, the Shepard sum and
// the neighbour count AT THE PARTICLES, on demand (sphmi_particle_fields).
//
// For every row i the handle holds, of any Type, over every row j ≠ i of any Type with r² = |x_i − x_j|² ≤ H² on the CURRENT positions:
//     V_j = m₀ / ρ_j        ∇ᵢW_ij = W′(r) · (x_i − x_j) / r        W: the handle's kernel (src/SPHKernels.jl:75-91), its αD and h
//     n = rows      S = V_i W(0) + Σ V_j W_ij      N = Σ V_j ∇ᵢW_ij      ∇·r = Σ V_j (x_j − x_i)·∇ᵢW_ij
//     ∇·v = Σ V_j (v_j − v_i)·∇ᵢW_ij      ω = Σ V_j ∇ᵢW_ij × (v_j − v_i)
// on the state sphmi_download would deliver now: Position and Density record + low word on fp32 handles, Velocity of the current
// set; no pressure.  A coincident row (r = 0) counts in n and S and adds nothing to the four gradient sums.  r² is
// ((dx² + dy²) + dz²) with contraction off, as in k_probe_sample: a row AT the cut is in or out for the kernel and a host reference
// alike.  Everything is summed in fp64.  With these signs a rigid rotation v = Ω × x gives ω = 2Ω; N is the gradient
// of the colour function Σ V_j W: at a free surface it points INTO the fluid, the outward normal is −N / |N|.
//
// k_particle_fields — k_field_grid (sphmi_field_grid.h) with a run of rows where that kernel has a brick of lattice nodes.  One
// workgroup of four waves takes 256 consecutive rows of the sorted order, one target per lane.
//   * Candidate rows: the workgroup's min / max over its targets' current positions take the place of the brick's first and last
//     node; the box is widened per axis by reach = H + h and the 1e-6 the probes derive ("EXACT, NOT STALE", sphmi_probes.h — the
//     derivation bounds how far a row j may lie from the cell it was hashed into, whatever the point it is looked up from, so it
//     holds for a target at its current position) and clamped to the grid.  By monotony of ceil / floor the span holds the
//     candidate cells of every target of the run: every target sees every row within H, however stale the cell list.  Per
//     (cy, cz) the x-adjacent cells are ONE range of `cstart`; the ranges are taken in (cz, cy, row) order, 256 per batch, and
//     concatenated by a workgroup scan.
//     (Rows are sorted x-fastest: a run that crosses the end of a row of cells has a box as long as the grid.  It still sees
//     exactly its rows, it just walks more candidates; at the headline size that is about one run in twelve.)
//   * Staging: chunks of 256 candidates, double buffered; lane t finds candidate 256·c + t by a binary search of the scan, loads
//     both packets (fp32: and the low words) and converts ONCE to { x, y, z, m₀/ρ, v, row index } in fp64 — eight doubles, 64 bytes.
//     Every row a single-device handle holds is live (N == capacity), so no row is staged as absent.
//   * Walk: every lane reads the staged rows in order — one LDS address for all lanes, a broadcast — applies the exact cut for its
//     own target and skips j = i by row index (read only behind the cut).
// The order of every sum is the row order (cz, cy, row): no atomics, no cross-lane reduction, the same bits on every call.  Lanes
// past N carry a NaN position: they fail every cut and write nothing.
//
// Results, in the layout the caller receives (the host copies what was asked for): n [N] int64, S [N], N [N × 3], ∇·r [N], ∇·v [N],
// ω [N × 3] — ten doubles per row, arrays back to back in the handle's arena.  2-D handles write exact zeros to N_z, ω_x and ω_y.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_kernels.h"
#include "sphmi_rebuild.h"

namespace sphmi {

constexpr int kPfThreads = 256;                  // targets of a run, candidates of a chunk, ranges of a batch
constexpr int kPfRow = 8;                        // doubles of a staged row: x, y, z, m₀/ρ, v[3], row index (int64 bits)
constexpr int kPfValues = 10;                    // doubles of a result row: n, S, N[3], ∇·r, ∇·v, ω[3]
constexpr size_t kPfLdsBytes = 2 * (size_t)kPfThreads * kPfRow * 8 + 2 * (size_t)kPfThreads * 4 + 4 * 6 * 8 + 64;

template <class T> struct ParticleFieldArgs {
    using V4 = typename Vec4<T>::type;
    Half<const V4> pk0, pk1;             // the set sphmi_download reads
    const V4* comp;                      // fp32 handles: low words of position and density (null: none)
    const int* cstart;
    long long* count;                    // the six result arrays (above)
    double *shepard, *normal, *div_r, *div_v, *vorticity;
    GridDesc g;
    double H_inv, H2, h_inv, reach;
    double alphaD, m0;
    int N, kernel;
};

// W(r) and W′(r) / r of src/SPHKernels.jl:75-87 (Wendland C2) and :89-105 (CubicSpline; the exact W′ / r, without the η² the
// reference adds to r) in fp64, q = r / h.  Wendland: W′ = −5 αD q (1 − q/2)³ / h, so W′ / r = −5 αD (1 − q/2)³ / h² without a
// division; the spline's inner branch likewise.  r = 0 gives a finite W′ / r: the caller multiplies it by x_i − x_j = 0.
__device__ __forceinline__ void pf_kernel(int kernel, double alphaD, double h_inv, double r, double& W, double& dW_r) {
    const double q = r * h_inv;
    if (kernel == 1) {                   // SPHMI_KERNEL_CUBIC_SPLINE
        const double t = 2.0 - q;
        if (q <= 1.0) { W = alphaD * (1.0 - 1.5 * q * q + 0.75 * q * q * q); dW_r = alphaD * h_inv * h_inv * (2.25 * q - 3.0); }
        else if (q <= 2.0) { W = alphaD * (0.25 * t * t * t); dW_r = alphaD * h_inv * (-0.75 * t * t) / r; }
        else { W = 0.0; dW_r = 0.0; }
        return;
    }
    const double t = 1.0 - 0.5 * q, t2 = t * t;
    W = alphaD * (t2 * t2) * (2.0 * q + 1.0);
    dW_r = -5.0 * alphaD * h_inv * h_inv * (t2 * t);
}

template <class T, int D>
__global__ void __launch_bounds__(kPfThreads, 4) k_particle_fields(const ParticleFieldArgs<T> A) {
    using V4 = typename Vec4<T>::type;
    __shared__ double s_row[2][kPfThreads * kPfRow];
    __shared__ int s_rs[kPfThreads], s_incl[kPfThreads];
    __shared__ double s_box[4][6];
    __shared__ int s_wave[4];
    static_assert(sizeof(s_row) + sizeof(s_rs) + sizeof(s_incl) + sizeof(s_box) + sizeof(s_wave) <= kPfLdsBytes, "LDS of k_particle_fields");
    static_assert(4 * kPfLdsBytes <= 160 * 1024, "four workgroups of k_particle_fields per compute unit");
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const double kNaN = __longlong_as_double(0x7ff8000000000000ll);

    // the target of this lane: position, velocity and volume as sphmi_download delivers them
    const long long i = (long long)blockIdx.x * kPfThreads + t;
    const bool has_row = i < (long long)A.N;
    double xi[3] = {kNaN, 0.0, 0.0}, vi[3] = {0.0, 0.0, 0.0}, Vi = 0.0;
    if (has_row) {
        const V4 q0 = A.pk0[i], q1 = A.pk1[i];
        V4 lw; lw.x = lw.y = lw.z = lw.w = T(0);
        if (sizeof(T) == 4 && A.comp) lw = A.comp[i];
        xi[0] = (double)q0.x + (double)lw.x; xi[1] = (double)q0.y + (double)lw.y; xi[2] = D == 3 ? (double)q0.z + (double)lw.z : 0.0;
        vi[0] = (double)q1.x; vi[1] = (double)q1.y; vi[2] = D == 3 ? (double)q1.z : 0.0;
        Vi = A.m0 / ((double)(q0.w < T(0) ? -q0.w : q0.w) + (double)lw.w);
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

    double n = 0.0, S = 0.0, Nx = 0.0, Ny = 0.0, Nz = 0.0, dr = 0.0, dv = 0.0, wx = 0.0, wy = 0.0, wz = 0.0;
    for (int rbase = 0; rbase < nrange; rbase += kPfThreads) {
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
        const int total = s_incl[kPfThreads - 1];
        const int nchunk = (total + kPfThreads - 1) / kPfThreads;

        V4 q0, q1, lw;
        int k = 0;
        auto load = [&](int c) {
            const int q = c * kPfThreads + t;
            k = 0;
            if (q < total) {
                int a = 0, b = kPfThreads - 1;               // the first range with s_incl > q
                while (a < b) { const int m = (a + b) >> 1; if (s_incl[m] > q) b = m; else a = m + 1; }
                k = s_rs[a] + q;
            }
            q0 = A.pk0[k]; q1 = A.pk1[k];
            if (sizeof(T) == 4 && A.comp) lw = A.comp[k]; else { lw.x = lw.y = lw.z = lw.w = T(0); }
        };
        auto stage = [&](int buf) {                          // (a lane past `total` stages row 0 again: the walk stops at `total`)
            double* r = &s_row[buf][t * kPfRow];
            r[0] = (double)q0.x + (double)lw.x;
            r[1] = (double)q0.y + (double)lw.y;
            r[2] = (double)q0.z + (double)lw.z;
            r[3] = A.m0 / ((double)(q0.w < T(0) ? -q0.w : q0.w) + (double)lw.w);
            r[4] = (double)q1.x; r[5] = (double)q1.y; r[6] = (double)q1.z;
            r[7] = __longlong_as_double((long long)k);
        };
        if (nchunk > 0) { load(0); stage(0); }
        __syncthreads();
        for (int c = 0; c < nchunk; ++c) {
            const bool more = c + 1 < nchunk;
            if (more) load(c + 1);                           // in flight while chunk c is walked
            const double* R = s_row[c & 1];
            const int cnt = min(kPfThreads, total - c * kPfThreads);
#pragma unroll 2
            for (int j = 0; j < cnt; ++j) {
                const double* r = R + j * kPfRow;
                double dx, dy, dz, r2;
                {
                    // (no contraction: r² is ((dx² + dy²) + dz²) rounded term by term, as in k_probe_sample)
#pragma clang fp contract(off)
                    dx = xi[0] - r[0]; dy = xi[1] - r[1]; dz = D == 3 ? xi[2] - r[2] : 0.0;
                    r2 = dx * dx + dy * dy + dz * dz;
                }
                if (r2 <= A.H2 && __double_as_longlong(r[7]) != i) {
                    double W, F;
                    pf_kernel(A.kernel, A.alphaD, A.h_inv, sqrt(r2), W, F);
                    const double Vj = r[3];
                    n += 1.0; S += Vj * W;
                    F *= Vj;                                 // V_j ∇ᵢW_ij = F · (dx, dy, dz); zero at r = 0
                    const double gx = F * dx, gy = F * dy, gz = F * dz;
                    const double ux = r[4] - vi[0], uy = r[5] - vi[1], uz = D == 3 ? r[6] - vi[2] : 0.0;
                    Nx += gx; Ny += gy;
                    dr -= gx * dx + gy * dy;
                    dv += ux * gx + uy * gy;
                    wz += gx * uy - gy * ux;
                    if (D == 3) {
                        Nz += gz; dr -= gz * dz; dv += uz * gz;
                        wx += gy * uz - gz * uy; wy += gz * ux - gx * uz;
                    }
                }
            }
            if (more) stage((c + 1) & 1);                    // the buffer chunk c − 1 was walked from: every lane is past the barrier behind it
            __syncthreads();
        }
    }
    if (has_row) {
        double W0, F0;
        pf_kernel(A.kernel, A.alphaD, A.h_inv, 0.0, W0, F0);
        A.count[i] = (long long)n;
        A.shepard[i] = Vi * W0 + S;
        A.normal[3 * i] = Nx; A.normal[3 * i + 1] = Ny; A.normal[3 * i + 2] = D == 3 ? Nz : 0.0;
        A.div_r[i] = dr; A.div_v[i] = dv;
        A.vorticity[3 * i] = D == 3 ? wx : 0.0; A.vorticity[3 * i + 1] = D == 3 ? wy : 0.0; A.vorticity[3 * i + 2] = wz;
    }
}

}  // namespace sphmi
