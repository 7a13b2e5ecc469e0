// sphmi_flow.h — the flow through control boxes at every step, recorded on the device (sphmi_flow_enable / _read): how much fluid
// a region holds and how much went in or out — the discharge through a section, overtopping, the filling curve of a compartment.
//
// A box is axis-aligned and half-open: row i is INSIDE box b iff lo[b][d] <= x_i[d] < hi[b][d] for every d < dims, compared in fp64
// on the Position doubles sphmi_download would deliver (delivered_coord, sphmi_step_record.h).  -inf and +inf are bounds like any
// other; a 2-D handle carries z = 0 and (-inf, +inf) on the third axis, so the same three comparisons serve both.  Only rows that
// count do (owned_fluid, the same header: the handle's own, Type == Fluid).
//
// The raw record of an EXECUTED step, kFlValues doubles per box, every slot a sum over the counting rows:
//     0        n_after    rows inside on the state a download delivers directly after the step
//     1        Σ 1/ρ      over those rows, one fp64 division per row
//     2–4      Σ v        over those rows (2-D: the third an exact zero)
//     5        entered    rows NOT inside on the state at the START of the step and inside after it
//     6        left       rows inside at the start of the step and not inside after it
// The host multiplies 1 and 2–4 by m₀ (deliver_flow, sphmi_series.h); a multi-device handle adds the slabs' records first.
//
// The state at the start of a step no longer exists behind its corrector: on fp32 handles the corrector updates the low words in
// place.  So the start state is MARKED before anything of the step runs:
//     k_fl_mark      the first launch of a step, one row per lane: a uint16 per row, bit b set iff the row counts and is inside box b
//                    on the current set + low words.  It does not look at StepCtrl::active — with the control fused into the
//                    predictor the step's decision has not been taken yet — a cancelled step leaves marks nobody reads.  Rebuilds
//                    permute rows BETWEEN steps, so the marks of a step and its sample see the same row order.
//     k_fl_partial   behind the corrector, on its output set; block b = rows 256·b … 256·b + 255, one row per lane.  Per box (a run-
//                    time loop, the bounds in the kernel arguments, nothing indexed per lane) a wave forms its three counts as
//                    __popcll(__ballot(...)) of the after / entered / left predicates, and the four floating-point sums by the
//                    butterfly wave_sum — only when the after-ballot is non-zero: a skipped box contributes +0.0, which
//                    is what the butterfly of sixty-four +0.0 identities yields, so skipping never changes a bit.  Then waves
//                    0, 1, 2, 3 in that order → partial[b][box][kFlValues].
//     k_fl_final     one workgroup of 64 per box: lane l takes the partials l, l + 64, … in order, then the same butterfly; box 0
//                    writes the header of the record.
//     k_fl_small     both stages in one launch of one workgroup, the partials in LDS, adding in exactly the same order (handles of
//                    at most kFlSmallRows rows, or $SPHMI_FLOW_SMALL_ROWS up to kFlSmallRowsMax): the same bits.
// The three samplers return at once when the step was cancelled (StepCtrl::active == 0).  No atomics; the order of every sum follows
// from the row order alone.  Every term is formed with contraction off: a host forms the same doubles from a download.
//
// Record (StepRecord, sphmi_step_record.h; kStepHeader + kFlValues · n_boxes doubles): the header, then the boxes' values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_kernels.h"
#include "sphmi_series.h"       // kMaxFlowBoxes, kFlValues
#include "sphmi_step_record.h"  // StepRecord, wave_sum, the delivered row

namespace sphmi {

constexpr int kFlBlock = 256;                    // rows of a partial = threads of the workgroup that forms it
constexpr int kFlSmallBlocks = 32;               // k_fl_small keeps the partials in LDS: this many blocks at most
constexpr int kFlSmallRowsMax = kFlSmallBlocks * kFlBlock;
constexpr int kFlSmallRows = 2 * kFlBlock;       // the budgets' threshold, until measured otherwise (profiles/flow.md)

// the boxes as the kernels see them: three axes each (2-D handles: the third is (-inf, +inf))
struct FlowBoxes {
    double lo[kMaxFlowBoxes][3], hi[kMaxFlowBoxes][3];
    int n;
};

template <class T> struct FlowArgs {
    using V4 = typename Vec4<T>::type;
    StepRecord step;                     // (k_fl_mark: unused)
    Half<const V4> pk0, pk1;             // k_fl_mark: the current set; the samplers: the corrector's output set
    const V4* comp;                      // fp32 handles: low words of position and density (null: none)
    const uint8_t* type;                 // slab handles: the type byte (ghost copies, dead rows); null on plain handles
    uint16_t* mark;                      // one per row: bit b = counted and inside box b at the start of the step
    double* partial;                     // n_boxes × kFlValues doubles per block of 256 rows
    int N, D, nblk;                      // nblk = ⌈N / 256⌉
    FlowBoxes box;
};

// what a lane needs of its row; `counts` = 0 for a lane past N and for a row that is not an owned Fluid row
template <class T> struct FlowRow {
    double x, y, z, vx, vy, vz, inv_rho;
    int counts;
};
// `full` = 0: the position alone (k_fl_mark)
// (`Args`: FlowArgs<T>, or whatever carries N, D, pk0, pk1, comp and type as it does — MapArgs<T>, sphmi_maps.h)
template <class T, class Args>
__device__ __forceinline__ FlowRow<T> fl_load(const Args& A, long long i, bool full) {
#pragma clang fp contract(off)
    using V4 = typename Vec4<T>::type;
    FlowRow<T> r;
    r.x = r.y = r.z = r.vx = r.vy = r.vz = r.inv_rho = 0.0;
    r.counts = 0;
    if (i >= (long long)A.N) return r;
    const V4 q0 = A.pk0[i];
    if (!owned_fluid(row_type(A.type, i, q0.w))) return r;
    V4 lw;
    lw.x = lw.y = lw.z = lw.w = T(0);
    if (sizeof(T) == 4 && A.comp) lw = A.comp[i];
    const bool three = A.D == 3;
    r.counts = 1;
    r.x = delivered_coord(q0.x, lw.x); r.y = delivered_coord(q0.y, lw.y); r.z = three ? delivered_coord(q0.z, lw.z) : 0.0;
    if (full) {
        const V4 q1 = A.pk1[i];
        r.vx = (double)q1.x; r.vy = (double)q1.y; r.vz = three ? (double)q1.z : 0.0;
        r.inv_rho = 1.0 / delivered_density(q0.w, lw.w);
    }
    return r;
}
// the half-open rule (b is the same in every lane: the bounds are scalar loads of the kernel arguments)
template <class T>
__device__ __forceinline__ bool fl_inside(const FlowArgs<T>& A, const FlowRow<T>& r, int b) {
    return r.counts && A.box.lo[b][0] <= r.x && r.x < A.box.hi[b][0] && A.box.lo[b][1] <= r.y && r.y < A.box.hi[b][1] &&
           A.box.lo[b][2] <= r.z && r.z < A.box.hi[b][2];
}

// the first launch of a step: the boxes every counting row is inside of NOW
template <class T>
__global__ void __launch_bounds__(kFlBlock) k_fl_mark(const FlowArgs<T> A) {
    const long long i = (long long)blockIdx.x * kFlBlock + (int)threadIdx.x;
    if (i >= (long long)A.N) return;
    const FlowRow<T> r = fl_load<T>(A, i, false);
    unsigned m = 0;
    for (int b = 0; b < A.box.n; ++b) m |= fl_inside<T>(A, r, b) ? 1u << b : 0u;
    A.mark[i] = (uint16_t)m;
}

// the workgroup's 256 threads reduce the rows they loaded; threads 0 … kFlValues · n_boxes − 1 write dst[box · kFlValues + slot]
// (s_w: 4 × kMaxFlowBoxes · kFlValues doubles of LDS, free again on return)
template <class T>
__device__ __forceinline__ void fl_block_reduce(const FlowArgs<T>& A, const FlowRow<T>& r, unsigned before, double (*s_w)[kMaxFlowBoxes * kFlValues],
                                                double* dst) {
#pragma clang fp contract(off)
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int b = 0; b < A.box.n; ++b) {
        const bool after = fl_inside<T>(A, r, b), was = (before >> b) & 1u;
        const unsigned long long in = __ballot(after);
        const double n_in = (double)__popcll(in), n_entered = (double)__popcll(__ballot(after && !was)), n_left = (double)__popcll(__ballot(was && !after));
        double s1 = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
        if (in != 0ull) {       // (wave-uniform; an empty wave would add sixty-four +0.0: the same +0.0)
            s1 = wave_sum(after ? r.inv_rho : 0.0);
            sx = wave_sum(after ? r.vx : 0.0); sy = wave_sum(after ? r.vy : 0.0); sz = wave_sum(after ? r.vz : 0.0);
        }
        if (lane == 0) {
            double* w = s_w[wave] + b * kFlValues;
            w[0] = n_in; w[1] = s1; w[2] = sx; w[3] = sy; w[4] = sz; w[5] = n_entered; w[6] = n_left;
        }
    }
    __syncthreads();
    if (tid < A.box.n * kFlValues) dst[tid] = ((s_w[0][tid] + s_w[1][tid]) + s_w[2][tid]) + s_w[3][tid];
    __syncthreads();
}

// one wave: box `b` of this step's record from the partials (global memory or LDS); box 0 writes the header
template <class T>
__device__ __forceinline__ void fl_write_box(const FlowArgs<T>& A, const StepCtrl& c, const double* partial, int nblk, int b) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x & 63;
    const long long slot = A.step.slot(c);
    if (slot < 0) return;
    double v[kFlValues];
#pragma unroll
    for (int k = 0; k < kFlValues; ++k) v[k] = 0.0;
    for (int blk = lane; blk < nblk; blk += 64) {
        const double* p = partial + ((size_t)blk * A.box.n + b) * kFlValues;
#pragma unroll
        for (int k = 0; k < kFlValues; ++k) v[k] = v[k] + p[k];
    }
#pragma unroll
    for (int k = 0; k < kFlValues; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0) {
        double* rec = A.step.at(slot);
        if (b == 0) A.step.write_header(rec, c);
#pragma unroll
        for (int k = 0; k < kFlValues; ++k) rec[kStepHeader + b * kFlValues + k] = v[k];
    }
}

// any grid: workgroup w takes blocks w, w + gridDim.x, …
template <class T>
__global__ void __launch_bounds__(kFlBlock) k_fl_partial(const FlowArgs<T> A) {
    if (!A.step.ctrl->active) return;
    __shared__ double s_w[4][kMaxFlowBoxes * kFlValues];
    for (int b = (int)blockIdx.x; b < A.nblk; b += (int)gridDim.x) {
        const long long i = (long long)b * kFlBlock + (int)threadIdx.x;
        const FlowRow<T> r = fl_load<T>(A, i, true);
        const unsigned before = i < (long long)A.N ? A.mark[i] : 0u;
        fl_block_reduce<T>(A, r, before, s_w, A.partial + (size_t)b * A.box.n * kFlValues);
    }
}
// grid = n_boxes workgroups of one wave
template <class T>
__global__ void __launch_bounds__(64) k_fl_final(const FlowArgs<T> A) {
    const StepCtrl c = *A.step.ctrl;
    if (!c.active || (int)blockIdx.x >= A.box.n) return;
    fl_write_box<T>(A, c, A.partial, A.nblk, (int)blockIdx.x);
}
// one workgroup: the blocks one after the other, the partials in LDS; wave w writes boxes w, w + 4, …
template <class T>
__global__ void __launch_bounds__(kFlBlock) k_fl_small(const FlowArgs<T> A) {
    const StepCtrl c = *A.step.ctrl;
    if (!c.active) return;
    __shared__ double s_w[4][kMaxFlowBoxes * kFlValues];
    __shared__ double s_partial[kFlSmallBlocks * kMaxFlowBoxes * kFlValues];
    const int nblk = min(A.nblk, kFlSmallBlocks);
    for (int b = 0; b < nblk; ++b) {
        const long long i = (long long)b * kFlBlock + (int)threadIdx.x;
        const FlowRow<T> r = fl_load<T>(A, i, true);
        const unsigned before = i < (long long)A.N ? A.mark[i] : 0u;
        fl_block_reduce<T>(A, r, before, s_w, s_partial + (size_t)b * A.box.n * kFlValues);
    }
    __syncthreads();
    for (int b = (int)threadIdx.x >> 6; b < A.box.n; b += 4) fl_write_box<T>(A, c, s_partial, nblk, b);
}

}  // namespace sphmi
