// sphmi_step_record.h — the device side the per-step observers share (sphmi_series.h is the host side).
//
// THE RECORD OF A STEP.  An observer that records once per executed step owns a log of `slots` records of `record` doubles, which
// travels with the control block of a batch.  The step whose corrector read `ctrl` writes slot steps_done − 1 − (steps done when
// the batch was queued): cancelled steps leave no holes, re-queued steps no duplicates.  A record opens with kStepHeader doubles
// { iteration (int64 bits), TotalTime at the end of the step, Δt }; its payload is the observer's.
//
// THE DELIVERED ROW.  The doubles sphmi_download would deliver directly after the step, as k_pack_output forms them: Position =
// record + low word (fp32 handles; 0 elsewhere), Density = |ρ·s| + low word — one fp64 addition of two converted values each,
// contraction off, so that no product of a caller fuses with it: a host forms the same doubles from a download.  A row COUNTS when
// the handle owns it and its Type is Fluid: slab handles keep a type byte (ghost copies, dead rows), plain handles read Fluid off
// the sign of the ρ·s slot.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_kernels.h"      // StepCtrl
#include "sphmi_rebuild.h"      // kTypeMask, kGhostMask
#include "sphmi_series.h"       // kStepHeader

namespace sphmi {

// by value in the kernel arguments of every per-step observer (Engine::step_record fills it)
struct StepRecord {
    const StepCtrl* ctrl;            // the block this step's corrector read
    double* log;                     // `slots` records of `record` doubles
    long long iteration0;            // SimMetaData.Iteration when this sphmi_advance began (StepCtrl::steps_done counts from there)
    long long steps_base;            // steps done when the batch of this step was queued
    int record, slots;
    // the slot of the step `c` describes, −1: the log of the batch has none for it
    __device__ __forceinline__ long long slot(const StepCtrl& c) const {
        const long long s = c.steps_done - 1 - steps_base;
        return s < 0 || s >= (long long)slots ? -1 : s;
    }
    __device__ __forceinline__ double* at(long long slot) const { return log + (size_t)slot * (size_t)record; }
    // one lane of the launch
    __device__ __forceinline__ void write_header(double* rec, const StepCtrl& c) const {
        rec[0] = __longlong_as_double(iteration0 + c.steps_done);
        rec[1] = c.total_time;
        rec[2] = c.last_dt;
    }
};

// `op` over the lanes of a wave, a fixed butterfly: every lane ends up with the same bits
template <class Op>
__device__ __forceinline__ double wave_butterfly(double v, Op&& op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
    return wave_butterfly(v, [](double a, double b) {
#pragma clang fp contract(off)
        return a + b;
    });
}

// the type byte of row i, whose ρ·s slot is `rho_s`
template <class T>
__device__ __forceinline__ uint8_t row_type(const uint8_t* type, long long i, T rho_s) {
    return type ? type[i] : (uint8_t)(rho_s > T(0) ? 1 : 2);
}
// SPHMI_FLUID, and the handle's own: neither dead nor a ghost copy
__device__ __forceinline__ bool owned_fluid(uint8_t ty) { return (ty & kTypeMask) == 1 && !(ty & kGhostMask); }

template <class T>
__device__ __forceinline__ double delivered_coord(T rec, T low) {
#pragma clang fp contract(off)
    return (double)rec + (double)low;
}
template <class T>
__device__ __forceinline__ double delivered_density(T rho_s, T low) {
#pragma clang fp contract(off)
    return (double)(rho_s < T(0) ? -rho_s : rho_s) + (double)low;
}

}  // namespace sphmi
