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
// k_point_moments — pc_walk (sphmi_point_cloud.h: the bins, the tile, the span, the staging and the cut are described there) over
// PcmSums.  n, S, SP, Sρ and Sv are formed by the statements of PcSums, so that they are the sums sphmi_sample_points and
// sphmi_sample_point_gradients deliver, bit for bit.
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

// the sums of a point and their moments, as one lane carries them through pc_walk (the constants: PcSums).  PmSums is the probes' set
// (sphmi_probe_moments.h): one wave per probe, every sum reduced over the wave; this one is a lane's own.
template <int D>
struct PcmSums {
    static constexpr bool kUniform = true, kUnroll2 = false;
    PcSums<D, int> z;                    // n, S, SP, Sρ, Sv: the cloud's own
    double M1[3] = {0.0, 0.0, 0.0}, P1[3] = {0.0, 0.0, 0.0}, R1[3] = {0.0, 0.0, 0.0};
    double M2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double V1[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    template <class Args>
    __device__ __forceinline__ void add(const Args& A, const double* r, double w, double dist, double dx, double dy, double dz) {
        // w e with e = x_j − x = −(dx, dy, dz): every moment is one product with it
        const double wx = w * -dx, wy = w * -dy, wz = w * -dz;
        const double rho = r[5];
        z.add(A, r, w, dist, dx, dy, dz);
        M1[0] += wx; M1[1] += wy;
        M2[0] += wx * -dx; M2[1] += wx * -dy; M2[3] += wy * -dy;
        P1[0] += r[4] * wx; P1[1] += r[4] * wy;
        R1[0] += rho * wx; R1[1] += rho * wy;
        V1[0][0] += r[6] * wx; V1[0][1] += r[6] * wy;
        V1[1][0] += r[7] * wx; V1[1][1] += r[7] * wy;
        if (D == 3) {
            M1[2] += wz;
            M2[2] += wx * -dz; M2[4] += wy * -dz; M2[5] += wz * -dz;
            P1[2] += r[4] * wz; R1[2] += rho * wz;
            V1[0][2] += r[6] * wz; V1[1][2] += r[7] * wz;
            V1[2][0] += r[8] * wx; V1[2][1] += r[8] * wy; V1[2][2] += r[8] * wz;
        }
    }
    __device__ __forceinline__ void store(double* o, long long M) const {
        z.store(o, M);
        // the slots below are the entries moment1, moment2, moment_pressure, moment_density and moment_velocity of kPmOutputs
        static_assert(kPmOutputs[3].first == 7 && kPmOutputs[4].first == 10 && kPmOutputs[5].first == 16 && kPmOutputs[6].first == 19 && kPmOutputs[7].first == 22,
                      "the stores of k_point_moments fill the slots of kPmOutputs");
        // (xx, xy, xz, yy, yz, zz: the entries with a z index are 2, 4 and 5)
        o[10 * M] = M2[0]; o[11 * M] = M2[1]; o[12 * M] = D == 3 ? M2[2] : 0.0;
        o[13 * M] = M2[3]; o[14 * M] = D == 3 ? M2[4] : 0.0; o[15 * M] = D == 3 ? M2[5] : 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const bool zero = b >= D;                        // a slot of the third axis on a 2-D handle: an exact zero
            o[(7 + b) * M] = zero ? 0.0 : M1[b];
            o[(16 + b) * M] = zero ? 0.0 : P1[b];
            o[(19 + b) * M] = zero ? 0.0 : R1[b];
#pragma unroll
            for (int a = 0; a < 3; ++a) o[(22 + 3 * a + b) * M] = (zero || a >= D) ? 0.0 : V1[a][b];
        }
    }
};

// the arguments are k_point_cloud's; `out` holds kPmValues arrays of n_points doubles
template <class T, int D>
__global__ void __launch_bounds__(kFgThreads, 2) k_point_moments(const PointCloudArgs<T> A) {
    const int t = (int)threadIdx.x;
    // the tile of this workgroup, the point of this lane
    const PcTile tile = A.tiles[blockIdx.x];
    const bool has_point = t < tile.count;
    // (the caller's index of the point is read here and AGAIN before the stores: it is not carried through the walk.  The empty asm
    // keeps the compiler from merging the two reads, which would carry the 64-bit slot instead.)
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
    PcmSums<D> s;
    pc_walk<T, D>(A, xp, has_point, s);
    if (has_point) s.store(A.out + caller_index(), A.n_points);
}

}  // namespace sphmi
