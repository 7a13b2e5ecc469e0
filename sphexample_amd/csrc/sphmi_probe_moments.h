// sphmi_probe_moments.h — the MOMENT sums of the kernel weights at fixed probe points on every step (sphmi_probe_moments_enable /
// _read): what a first-order least-squares fit needs (sphexample_amd/fields.py: linear_fit; sphexample_amd/probes.py: fit_series), at
// step resolution — a pressure sensor on a wall, where the Shepard mean of sphmi_probes_enable reads the field a fraction of h inside
// the fluid.
//
// For every EXECUTED step and every probe p at the fixed position x_p, over the rows j the handle owns with Type == Fluid and
// r² = ((dx² + dy²) + dz²) ≤ H² on the CURRENT positions, contraction off, with w_j = (m₀ / ρ_j) W(r) and e_j = x_j − x_p:
//     n = rows      S = Σ w      SP = Σ w P      Sρ = Σ w ρ      Sv[a] = Σ w v[a]
//     M1[b] = Σ w e[b]      M2[bc] = Σ w e[b] e[c]  (xx, xy, xz, yy, yz, zz)
//     P1[b] = Σ w P e[b]    R1[b] = Σ w ρ e[b]      V1[a][b] = Σ w v[a] e[b]
// on the state sphmi_download would deliver directly after that step — the sums of sphmi_point_moments.h at the state of
// sphmi_probes.h.  Everything is fp64, there is no self term, a row at r = 0 adds nothing to the moments.  The RAW sums are recorded
// and delivered; a multi-device handle adds the slabs' records in slab order (every sum is linear in the rows).
//
// k_probe_moments — one wave per probe, queued behind every corrector next to k_probe_sample (Engine::pm_sample): returns at once on
// a cancelled step and writes this step's record of its OWN log.  The walk is pr_walk (sphmi_probes.h) and nothing else: the
// candidate cells with reach H + h that cover stale lists, up to 5 × 5 (cy, cz) ranges, jobs of 64 rows in (cz, cy, row) order, the
// fp64 cut with contraction off.  PmSums below is the set of sums it runs over.
//   * n, S, SP, Sρ and Sv are PrSums' own statements (PmSums calls them): slots 0 … 6 of a moment record equal the record of
//     k_probe_sample at the same point and step, bit for bit.
//   * The moment terms are formed as k_point_moments forms them — wx = w * -dx, M2 += wx * -dx, P1 += P * wx, … — every product
//     rounded before its addition (contraction off), so that the order of the additions alone decides the bits.
//   * Each lane adds its rows in job order, then one fixed butterfly (wave_sum) per sum: no atomics, repeated runs give the same
//     bits.  k_point_moments adds in ascending row order per lane, without a butterfly: the two kernels agree to the bar of
//     their tests (1e-10 of a sum's largest magnitude on fp64 handles), NOT to the bit.
//
// Budget, read off the code object by tests/test_probe_moments_host.py.  A lane carries 31 fp64 sums (62 registers) beside the
// loads in flight: 13 (fp32 records) or 18 (fp64) registers per job.  __launch_bounds__(256) — one wave per SIMD, as k_probe_sample
// is launched — leaves a lane 512 registers: with four jobs in flight the kernel takes 156 (fp32 records) / 158 (fp64), with eight
// 220 / 222, either way without scratch.  No LDS.  Eight against four, 256 probes on the bench case, three interleaved repetitions
// (profiles/probe_moments.md): +35 against +38 µs per step at rest, +61 against +55 µs in developed flow, each pair inside the
// spread of its runs — nothing to buy with the extra registers, so the kernel keeps the probes' four.
//
// Record (kStepHeader + kPmValues · n_probes doubles): the header, then per probe the kPmValues slots of sphmi_point_moments.h —
// { S, SP, Sρ, Sv[0..2], n }, M1 at 7, M2 at 10, P1 at 16, R1 at 19, V1[a][b] at 22 + 3a + b.  2-D handles write exact zeros to every
// slot of the third axis.  The host reads this layout from kPmOutputs (sphmi_series.h: deliver_probe_moments).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_probes.h"       // ProbeSampleArgs, PrSums, pr_walk
#include "sphmi_series.h"       // kMaxProbes, kPmValues, kPmOutputs
#include "sphmi_step_record.h"  // StepRecord, wave_sum

namespace sphmi {

constexpr int kPmRecordMax = kStepHeader + kPmValues * kMaxProbes;
constexpr int kPmInFlight = kPrInFlight; // jobs whose loads are issued before the first is used: the probes' four (the budget above)

static_assert(kPmValues == kPrValues + 24, "the sums of k_probe_sample, then M1, M2, P1, R1 and V1");

// the sums of a probe and their moments, as one lane carries them through pr_walk
struct PmSums {
    static constexpr int kInFlight = kPmInFlight;
    PrSums z;                            // n, S, SP, Sρ, Sv: the probes' own
    double M1[3] = {0.0, 0.0, 0.0}, P1[3] = {0.0, 0.0, 0.0}, R1[3] = {0.0, 0.0, 0.0};
    double M2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double V1[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    __device__ __forceinline__ void add(double w, double P, double rho, double vx, double vy, double vz, double dx, double dy, double dz) {
#pragma clang fp contract(off)
        z.add(w, P, rho, vx, vy, vz, dx, dy, dz);
        // w e with e = x_j − x_p = −(dx, dy, dz): every moment is one product with it
        const double wx = w * -dx, wy = w * -dy, wz = w * -dz;
        M1[0] += wx; M1[1] += wy; M1[2] += wz;
        M2[0] += wx * -dx; M2[1] += wx * -dy; M2[2] += wx * -dz; M2[3] += wy * -dy; M2[4] += wy * -dz; M2[5] += wz * -dz;
        P1[0] += P * wx; P1[1] += P * wy; P1[2] += P * wz;
        R1[0] += rho * wx; R1[1] += rho * wy; R1[2] += rho * wz;
        V1[0][0] += vx * wx; V1[0][1] += vx * wy; V1[0][2] += vx * wz;
        V1[1][0] += vy * wx; V1[1][1] += vy * wy; V1[1][2] += vy * wz;
        V1[2][0] += vz * wx; V1[2][1] += vz * wy; V1[2][2] += vz * wz;
    }
    __device__ __forceinline__ void reduce() {
        z.reduce();
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            M1[b] = wave_sum(M1[b]); P1[b] = wave_sum(P1[b]); R1[b] = wave_sum(R1[b]);
#pragma unroll
            for (int a = 0; a < 3; ++a) V1[a][b] = wave_sum(V1[a][b]);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) M2[k] = wave_sum(M2[k]);
    }
};

// the arguments are k_probe_sample's; `step` is the log of the moments, `pos` and `n_probes` their own point set
template <class T>
__global__ void __launch_bounds__(256) k_probe_moments(const ProbeSampleArgs<T> A) {
    const StepCtrl c = *A.step.ctrl;
    if (!c.active) return;
    const long long slot = A.step.slot(c);
    if (slot < 0) return;
    const int lane = (int)threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (p >= A.n_probes) return;
    double* rec = A.step.at(slot);
    if (p == 0 && lane == 0) A.step.write_header(rec, c);
    const double xp[3] = {A.pos[3 * p], A.pos[3 * p + 1], A.D == 3 ? A.pos[3 * p + 2] : 0.0};
    PmSums m;
    pr_walk<T>(A, xp, lane, m);
    if (lane == 0) {
        double* v = rec + kStepHeader + (size_t)kPmValues * p;
        const bool three = A.D == 3;
        v[0] = m.z.S; v[1] = m.z.SP; v[2] = m.z.Sr; v[3] = m.z.Sx; v[4] = m.z.Sy; v[5] = three ? m.z.Sz : 0.0; v[6] = m.z.n;
        // the slots below are the entries moment1, moment2, moment_pressure, moment_density and moment_velocity of kPmOutputs
        static_assert(kPmOutputs[3].first == 7 && kPmOutputs[4].first == 10 && kPmOutputs[5].first == 16 && kPmOutputs[6].first == 19 && kPmOutputs[7].first == 22,
                      "the stores of k_probe_moments fill the slots of kPmOutputs");
        // (xx, xy, xz, yy, yz, zz: the entries with a z index are 2, 4 and 5)
        v[10] = m.M2[0]; v[11] = m.M2[1]; v[12] = three ? m.M2[2] : 0.0;
        v[13] = m.M2[3]; v[14] = three ? m.M2[4] : 0.0; v[15] = three ? m.M2[5] : 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const bool zero = b >= A.D;                      // a slot of the third axis on a 2-D handle: an exact zero
            v[7 + b] = zero ? 0.0 : m.M1[b];
            v[16 + b] = zero ? 0.0 : m.P1[b];
            v[19 + b] = zero ? 0.0 : m.R1[b];
#pragma unroll
            for (int a = 0; a < 3; ++a) v[22 + 3 * a + b] = (zero || a >= A.D) ? 0.0 : m.V1[a][b];
        }
    }
}

}  // namespace sphmi
