// sphmi_envelopes.h — what every single particle has experienced over time, accumulated on the device at every step
// (sphmi_envelopes_enable / _read): the peak pressure a wall particle has seen, when the wave reached it and the impulse it took —
// the load MAP of a structure, not only its total — and the largest speed a fluid particle ever had.  Such peaks last a few steps;
// an output interval holds hundreds.
//
// The record of a row, kEnValues doubles (64 bytes), kept in the row order AT ENABLE and never moved.  With P the Pressure and v
// the Velocity sphmi_download would deliver directly after an executed step (P = Pressure!(ρₙ⁺) in the handle's arithmetic, eos7 —
// the function k_pack_output forms it with — widened; v widened, 2-D handles: vz = 0), t = StepCtrl::total_time at the end of that
// step and dt = StepCtrl::last_dt:
//     slot  value                          start   update per executed step
//     0     p_max                          −inf    if (P > p_max) { p_max = P; t_p_max = t; }     strict: the first attainment keeps its time
//     1     t_p_max                        0       (with slot 0)
//     2     p_min                          +inf    if (P < p_min) p_min = P
//     3     impulse = Σ P·dt               0       impulse = impulse + P * dt
//     4     square  = Σ P²·dt              0       square = square + (P * P) * dt
//     5     loaded  = Σ dt over P > 0      0       if (P > 0) loaded = loaded + dt
//     6     speed2_max = max |v|²          0       s = (vx*vx + vy*vy) + vz*vz; if (s > speed2_max) speed2_max = s
//     7     t_arrival                      +inf    if (P > 0 && t_arrival == inf) t_arrival = t
// Every operation is fp64, rounded once, contraction off: a host forms the same doubles from per-step downloads
// (sphexample_amd/envelopes.py: update).  A NaN never wins a comparison and poisons the sums.  There is no sqrt here: the host
// delivers sqrt(speed2_max) (deliver_envelope_speed, sphmi_series.h).
//
// The sort moves rows at every rebuild; the records stay and are FOUND, as the caller's passive columns are (sphmi_columns.h): the
// 4-byte row column the sorts carry anyway (Engine::prow) and a `base` map of the envelopes' own,
//     record of current row i  =  base[prow[i]]
// k_columns_base_init at enable, k_columns_base_compose in sphmi_download_permutation, k_gather_columns with a table of eight
// 8-byte columns at read — this header adds the first WRITER through that indirection.
//
//   k_en_fill     enable: the start record into every row's slot, the window header { 0 steps, t_begin, t_end = t_begin, 0 }
//   k_en_update   behind the corrector of every queued step, one row per lane; returns at once when the step was cancelled
//                 (StepCtrl::active == 0).  Two packets of the corrector's output set (the type off the sign of the ρ·s slot, as
//                 row_type of sphmi_step_record.h reads it; v), the density slot of the half-step set (P), prow[i], base[…] — both indices range-tested, as
//                 the column kernels test them: a corrupted column must not become a wild store — then the record with four 16-byte
//                 loads and at most four 16-byte stores (the pairs { p_max, t_p_max } and { speed2_max, t_arrival } only when they
//                 changed: late in a run they rarely do).  A row whose Type is not selected is left alone and keeps the start
//                 record.  dt and t are scalar loads of the control block; nothing is indexed per lane; no atomics — every record
//                 has exactly one writer.  Lane 0 of workgroup 0 updates the window header { steps, t_begin, t_end, duration = Σ dt
//                 in step order }.
// At rest the records of a wave are 4 KB in a row; late in a run the record order is random with respect to the row order and
// every lane touches a 64-byte half line of its own (profiles/envelopes.md has both).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_kernels.h"      // StepCtrl, Half, Vec4, eos7
#include "sphmi_series.h"       // kEnValues, kEnHeader

namespace sphmi {

constexpr int kEnBlock = 256;

template <class T> struct EnvelopeArgs {
    using V4 = typename Vec4<T>::type;
    const StepCtrl* ctrl;                // the block this step's corrector read
    Half<const V4> pk0, pk1;             // the corrector's output set
    Half<const V4> half0;                // the half-step set: Pressure is Pressure!(ρₙ⁺), as k_pack_output delivers it
    const int* prow;                     // row at the last sphmi_download_permutation
    const int* base;                     // row of that epoch → record
    double2* store;                      // N records of kEnValues doubles, then the window header
    double* header;                      // { steps (int64 bits), t_begin, t_end, duration }
    T rho0, inv_rho0, Cbe;
    unsigned type_mask;                  // bit Type: Fluid = 1, Fixed = 2 (every non-Fluid row of a plain handle carries 2 or 3: see `type`)
    const uint8_t* type;                 // the type byte: read only when the mask tells Fixed and Moving apart (null: never)
    int N, D;
};

__global__ void __launch_bounds__(kEnBlock) k_en_fill(double2* __restrict__ store, double* __restrict__ header, int n, double t_begin) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        header[0] = __longlong_as_double(0ll); header[1] = t_begin; header[2] = t_begin; header[3] = 0.0;
    }
    if (i >= n) return;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double2* r = store + (size_t)i * (kEnValues / 2);
    r[0] = double2{-inf, 0.0};
    r[1] = double2{inf, 0.0};
    r[2] = double2{0.0, 0.0};
    r[3] = double2{0.0, inf};
}

template <class T>
__global__ void __launch_bounds__(kEnBlock) k_en_update(const EnvelopeArgs<T> A) {
#pragma clang fp contract(off)
    using V4 = typename Vec4<T>::type;
    if (!A.ctrl->active) return;
    const double t = A.ctrl->total_time, dt = A.ctrl->last_dt;
    const long long i = (long long)blockIdx.x * kEnBlock + (int)threadIdx.x;
    if (i == 0) {
        // the window: one lane of the launch (the launches of a stream run in step order)
        A.header[0] = __longlong_as_double(__double_as_longlong(A.header[0]) + 1ll);
        A.header[2] = t;
        A.header[3] = A.header[3] + dt;
    }
    if (i >= (long long)A.N) return;
    const V4 q0 = A.pk0[i];
    // plain handles: Fluid off the sign of the ρ·s slot (row_type, sphmi_step_record.h); Fixed against Moving needs the type byte
    const unsigned ty = q0.w > T(0) ? 1u : (A.type ? (unsigned)A.type[i] & 3u : 2u);
    if (!((A.type_mask >> ty) & 1u)) return;
    const unsigned e = (unsigned)A.prow[i];
    if (e >= (unsigned)A.N) return;
    const unsigned s = (unsigned)A.base[e];
    if (s >= (unsigned)A.N) return;
    const V4 q1 = A.pk1[i];
    const double P = (double)eos7<T>(A.half0[i].w, A.rho0, A.inv_rho0, A.Cbe);
    const double vx = (double)q1.x, vy = (double)q1.y, vz = A.D == 3 ? (double)q1.z : 0.0;
    const double s2 = (vx * vx + vy * vy) + vz * vz;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);

    double2* r = A.store + (size_t)s * (kEnValues / 2);
    double2 a = r[0], b = r[1], c = r[2], d = r[3];
    if (P > a.x) { a.x = P; a.y = t; r[0] = a; }
    if (P < b.x) b.x = P;
    b.y = b.y + P * dt;
    r[1] = b;
    c.x = c.x + (P * P) * dt;
    if (P > 0.0) c.y = c.y + dt;
    r[2] = c;
    const bool faster = s2 > d.x, arrived = P > 0.0 && d.y == inf;
    if (faster) d.x = s2;
    if (arrived) d.y = t;
    if (faster || arrived) r[3] = d;
}

}  // namespace sphmi
