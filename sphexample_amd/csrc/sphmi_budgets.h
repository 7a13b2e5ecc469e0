// sphmi_budgets.h — the global budgets of the fluid at every step, recorded on the device (sphmi_budgets_enable / _read): kinetic,
// potential and compressive energy, linear and angular momentum, centre of mass, the largest speed, the density extremes and the
// bounding box (its maximum along x is the wave front of a dam break).
//
// For every EXECUTED step, over the rows that count (owned_fluid, sphmi_step_record.h: the handle's own, Type == Fluid), on the row
// a download would deliver directly after that step (the same header: delivered_coord, delivered_density; v = Velocity widened);
// 2-D handles have z = 0 and vz = 0.  The raw record, kBgValues doubles:
//     0        n                                    sum        10–12    Σ x                                 sum
//     1        Σ ½·((vx·vx + vy·vy) + vz·vz)        sum        13       max ((vx·vx + vy·vy) + vz·vz)       max
//     2        Σ x_last (the gravity axis)          sum        14, 15   min ρ, max ρ                        min, max
//     3        Σ e(ρ)                               sum        16–18    min x per axis (2-D: third 0)       min
//     4–6      Σ v                                  sum        19–21    max x per axis (2-D: third 0)       max
//     7–9      Σ x × v  (2-D: 7, 8 exact zeros)     sum
// e(ρ) = ((r6 − 1)/6 + 1/r) − 1 with r = ρ/ρ₀, r2 = r·r, r6 = (r2·r2)·r2: the compressive energy per unit mass of the Tait equation
// the engine runs (γ = 7, B = c₀²ρ₀/7), ∫ P/ρ² dρ from ρ₀, divided by B/ρ₀ — the host multiplies it back (deliver_budgets,
// sphmi_series.h), as it forms energies, momenta and the centre of mass from the raw sums (a multi-device handle combines the
// slabs' raw records first).  A record with n = 0 holds 0 in the sum slots, +inf in the min slots and −inf in the max slots.
//
// Every product and sum of a TERM is one fp64 operation of its own, in the order written, contraction off — as r² in
// k_particle_fields and for the reason the header of sphmi_field_grid.h gives: a host forms the same doubles from a download.
//
// Reduction, after the model of k_gf_partial / k_gf_final / k_gf_small (sphmi_group_forces.h): a fixed order, no atomics on
// floating-point values, nothing depends on the grid of the launch.
//     k_bg_partial   block b = rows 256·b … 256·b + 255, one row per lane (the identity where the row does not count): one butterfly
//                    over the 64 lanes, then waves 0, 1, 2, 3 in that order → partial[b][kBgValues]
//     k_bg_final     one wave: lane l takes the partials l, l + 64, … in order, then the same butterfly; the record of the step
//     k_bg_small     both stages in one launch of one workgroup, the partials in LDS, adding in exactly the same order (handles of
//                    at most kBgSmallRows rows, or $SPHMI_BUDGETS_SMALL_ROWS up to kBgSmallRowsMax)
// All three return at once when the step was cancelled (StepCtrl::active == 0).
//
// Record (StepRecord, sphmi_step_record.h; kStepHeader + kBgValues doubles): the header, then the 22 values above.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_kernels.h"
#include "sphmi_series.h"       // kBgValues, bg_rule
#include "sphmi_step_record.h"  // StepRecord, wave_butterfly, the delivered row

namespace sphmi {

constexpr int kBgBlock = 256;                    // rows of a partial = threads of the workgroup that forms it
constexpr int kBgRecord = kStepHeader + kBgValues;
constexpr int kBgSmallBlocks = 32;               // k_bg_small keeps the partials in LDS: this many blocks at most
constexpr int kBgSmallRowsMax = kBgSmallBlocks * kBgBlock;
// One workgroup reduces its blocks one after the other, every butterfly a chain of cross-lane exchanges nothing hides: measured
// ≈6 µs per block against 13.6 µs for the two-stage pair whatever the size (profiles/budgets.md) — one launch pays up to two blocks.
constexpr int kBgSmallRows = 2 * kBgBlock;
constexpr int kBgFinalInFlight = 4;              // partials whose loads k_bg_final issues before it adds the first

template <class T> struct BudgetArgs {
    using V4 = typename Vec4<T>::type;
    StepRecord step;                     // records of kBgRecord doubles
    Half<const V4> pk0, pk1;             // the corrector's output set
    const V4* comp;                      // fp32 handles: low words of position and density (null: none)
    const uint8_t* type;                 // slab handles: the type byte (ghost copies, dead rows); null on plain handles
    double* partial;                     // kBgValues doubles per block of 256 rows
    double rho0;
    int N, D, nblk;                      // nblk = ⌈N / 256⌉
};

__device__ __forceinline__ double bg_identity(int slot) {
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    return bg_rule(slot) == 0 ? 0.0 : (bg_rule(slot) == 1 ? inf : -inf);
}
__device__ __forceinline__ double bg_op(int slot, double a, double b) {
    return bg_rule(slot) == 0 ? a + b : (bg_rule(slot) == 1 ? fmin(a, b) : fmax(a, b));
}
// slot `slot` over the lanes of a wave, a fixed butterfly: every lane ends up with the same bits
__device__ __forceinline__ double bg_wave(int slot, double v) {
    return wave_butterfly(v, [slot](double a, double b) { return bg_op(slot, a, b); });
}

// what a lane reads of its row (a lane past N reads nothing: `has` = 0)
template <class T> struct BudgetRow {
    typename Vec4<T>::type q0, q1, lw;
    uint8_t ty, has;
};
template <class T>
__device__ __forceinline__ BudgetRow<T> bg_load(const BudgetArgs<T>& A, long long i) {
    BudgetRow<T> r;
    r.lw.x = r.lw.y = r.lw.z = r.lw.w = T(0);
    r.q0 = r.q1 = r.lw;
    r.ty = 0; r.has = i < (long long)A.N ? 1 : 0;
    if (r.has) {
        r.q0 = A.pk0[i]; r.q1 = A.pk1[i];
        if (sizeof(T) == 4 && A.comp) r.lw = A.comp[i];
        r.ty = row_type(A.type, i, r.q0.w);
    }
    return r;
}
// the terms of a row, or the identity of every slot when the row does not count
template <class T>
__device__ __forceinline__ void bg_terms(const BudgetArgs<T>& A, const BudgetRow<T>& r, double v[kBgValues]) {
#pragma unroll
    for (int k = 0; k < kBgValues; ++k) v[k] = bg_identity(k);
    if (!r.has || !owned_fluid(r.ty)) return;
    {
        // (no contraction: every product and sum is rounded on its own, the doubles a host forms from the download)
#pragma clang fp contract(off)
        const bool three = A.D == 3;
        const double x = delivered_coord(r.q0.x, r.lw.x), y = delivered_coord(r.q0.y, r.lw.y), z = three ? delivered_coord(r.q0.z, r.lw.z) : 0.0;
        const double vx = (double)r.q1.x, vy = (double)r.q1.y, vz = three ? (double)r.q1.z : 0.0;
        const double rho = delivered_density(r.q0.w, r.lw.w);
        const double v2 = (vx * vx + vy * vy) + vz * vz;
        const double rr = rho / A.rho0, r2 = rr * rr, r6 = (r2 * r2) * r2;
        v[0] = 1.0;
        v[1] = 0.5 * v2;
        v[2] = three ? z : y;
        v[3] = ((r6 - 1.0) / 6.0 + 1.0 / rr) - 1.0;
        v[4] = vx; v[5] = vy; v[6] = vz;
        v[7] = three ? y * vz - z * vy : 0.0;
        v[8] = three ? z * vx - x * vz : 0.0;
        v[9] = x * vy - y * vx;
        v[10] = x; v[11] = y; v[12] = z;
        v[13] = v2;
        v[14] = rho; v[15] = rho;
        v[16] = x; v[17] = y; v[18] = z;
        v[19] = x; v[20] = y; v[21] = z;
    }
}

// the workgroup's 256 threads reduce the rows they loaded; threads 0 … kBgValues − 1 write dst[slot] (s_w: 4 × kBgValues doubles of
// LDS, free again on return)
template <class T>
__device__ __forceinline__ void bg_block_reduce(const BudgetArgs<T>& A, const BudgetRow<T>& r, double (*s_w)[kBgValues], double* dst) {
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double v[kBgValues];
    bg_terms<T>(A, r, v);
#pragma unroll
    for (int k = 0; k < kBgValues; ++k) {
        const double s = bg_wave(k, v[k]);
        if (lane == 0) s_w[wave][k] = s;
    }
    __syncthreads();
    if (tid < kBgValues) dst[tid] = bg_op(tid, bg_op(tid, bg_op(tid, s_w[0][tid], s_w[1][tid]), s_w[2][tid]), s_w[3][tid]);
    __syncthreads();
}

// one wave: the record of this step from the partials (global memory or LDS)
template <class T>
__device__ __forceinline__ void bg_write_record(const BudgetArgs<T>& A, const StepCtrl& c, const double* partial, int nblk) {
    const int lane = (int)threadIdx.x & 63;
    const long long slot = A.step.slot(c);
    if (slot < 0) return;
    double v[kBgValues];
#pragma unroll
    for (int k = 0; k < kBgValues; ++k) v[k] = bg_identity(k);
    // (the loads of kBgFinalInFlight partials are issued together, a partial past the end is the identity; the adds keep their order)
    for (int b0 = lane; b0 < nblk; b0 += 64 * kBgFinalInFlight) {
        double p[kBgFinalInFlight][kBgValues];
#pragma unroll
        for (int u = 0; u < kBgFinalInFlight; ++u) {
            const int b = b0 + 64 * u;
#pragma unroll
            for (int k = 0; k < kBgValues; ++k) p[u][k] = b < nblk ? partial[(size_t)b * kBgValues + k] : bg_identity(k);
        }
#pragma unroll
        for (int u = 0; u < kBgFinalInFlight; ++u) {
#pragma unroll
            for (int k = 0; k < kBgValues; ++k) v[k] = bg_op(k, v[k], p[u][k]);
        }
    }
#pragma unroll
    for (int k = 0; k < kBgValues; ++k) v[k] = bg_wave(k, v[k]);
    if (lane == 0) {
        double* rec = A.step.at(slot);
        A.step.write_header(rec, c);
#pragma unroll
        for (int k = 0; k < kBgValues; ++k) rec[kStepHeader + k] = v[k];
    }
}

// any grid: workgroup w takes blocks w, w + gridDim.x, …
template <class T>
__global__ void __launch_bounds__(kBgBlock) k_bg_partial(const BudgetArgs<T> A) {
    if (!A.step.ctrl->active) return;
    __shared__ double s_w[4][kBgValues];
    for (int b = (int)blockIdx.x; b < A.nblk; b += (int)gridDim.x) {
        const BudgetRow<T> r = bg_load<T>(A, (long long)b * kBgBlock + (int)threadIdx.x);
        bg_block_reduce<T>(A, r, s_w, A.partial + (size_t)b * kBgValues);
    }
}
template <class T>
__global__ void __launch_bounds__(64) k_bg_final(const BudgetArgs<T> A) {
    const StepCtrl c = *A.step.ctrl;
    if (!c.active) return;
    bg_write_record<T>(A, c, A.partial, A.nblk);
}
// one workgroup: the blocks one after the other (the rows of the next one are in flight while one is reduced), the partials in LDS,
// wave 0 writes the record
template <class T>
__global__ void __launch_bounds__(kBgBlock) k_bg_small(const BudgetArgs<T> A) {
    const StepCtrl c = *A.step.ctrl;
    if (!c.active) return;
    __shared__ double s_w[4][kBgValues];
    __shared__ double s_partial[kBgSmallBlocks * kBgValues];
    const int nblk = min(A.nblk, kBgSmallBlocks);
    BudgetRow<T> r = bg_load<T>(A, (long long)threadIdx.x);
    for (int b = 0; b < nblk; ++b) {
        const BudgetRow<T> next = bg_load<T>(A, b + 1 < nblk ? (long long)(b + 1) * kBgBlock + (int)threadIdx.x : (long long)A.N);
        bg_block_reduce<T>(A, r, s_w, s_partial + b * kBgValues);
        r = next;
    }
    __syncthreads();
    if (threadIdx.x < 64) bg_write_record<T>(A, c, s_partial, nblk);
}

}  // namespace sphmi
