// sphmi_tracers.h — where the water goes: chosen particles followed, and massless drifters advected with the flow, on the device at
// every step (sphmi_tracers_enable / _read).  Probes sample at fixed points, the envelopes keep the extremes of a row but not its path;
// a pathline, a residence time or the fate of the water that overtops an obstacle needs the position at step resolution.
//
// Two kinds of tracer share ONE per-step series; either kind may be absent.  The record of an executed step (StepRecord,
// sphmi_step_record.h; kStepHeader + kTrParticleValues · n_particles + kTrDrifterValues · n_drifters doubles):
//     { the header,
//       { x[3], v[3], ρ, P }[tracked particle s],                          — the state AFTER the step
//       { X[3], S, SP, Sρ, Sv[3], n }[drifter p] }                         — X the position the sums were taken AT, before the move
//
// TRACKED PARTICLES — k_tr_particles, one row per lane over all rows.  The eight doubles are the values sphmi_download would deliver
// into Float64 host arrays directly after that step, bit for bit: Position and Density (delivered_coord, delivered_density of
// sphmi_step_record.h), Velocity, Pressure = Pressure!(ρₙ⁺) of the half-step set through eos7, as k_pack_output and the
// envelopes form it; 2-D handles store a zero third component.  A tracked row is found again after every sort the way the envelopes
// find their records (sphmi_envelopes.h, sphmi_columns.h), with a map of the tracers' own from the CURRENT row to the slot:
//     slot of current row i  =  slot_of_record[prow[i]]        (−1: not tracked)
// k_tr_map_init at enable (slot_of_record[prow[row_s]] = s over a table of −1), k_columns_base_compose in
// sphmi_download_permutation.  Both indices are range-tested before they are used, as k_en_update tests them: a corrupted column must
// not become a wild store.  A slot has exactly one writer (the rows of the enable are distinct); there are no atomics.
//
// DRIFTERS — k_tr_drift, one wave per drifter, behind the corrector of every executed step k.  With X_{k−1} the drifter's position
// before the step and the state after step k:
//     1. the probes' raw sums S, SP, Sρ, Sv[3], n at X_{k−1}: pr_walk (sphmi_probes.h) — the candidate cells, the reach H + h, the
//        inclusive cut r² ≤ H² with contraction off, the jobs of 64 rows, the fixed butterfly and the skipping of non-Fluid, dead and
//        ghost rows are k_probe_sample's, because it is the same function;
//     2. if (S >= min_weight) { U_d = Sv_d / S;  X_k[d] = X_{k−1}[d] + U_d * dt }  for d < dims, dt = StepCtrl::last_dt; every
//        operation fp64, rounded once, contraction off — a host forms the same doubles from the record (sphexample_amd/tracers.py:
//        step).  Otherwise the drifter is DRY and X_k = X_{k−1}: a drifter in empty space, above the surface or outside the dense grid
//        (empty ranges: S = 0, n = 0) stays where it is;
//     3. the record { X_{k−1}[3], S, SP, Sρ, Sv[3], n }: a complete probe sample at a known point.
// The scheme is FIRST ORDER (explicit Euler with the Shepard-mean velocity of the end state), like the tracer advection of comparable
// codes; the error of a pathline is O(Δt) per unit time, and Δt is the CFL step of the run.
// X lives in a buffer of its own (3 doubles per drifter) and is updated in place by lane 0 of the drifter's wave — the only reader
// and the only writer of its three doubles.  The move does not depend on the log: where the probes return before doing anything
// when the batch's log has no slot left, here the `slot` test guards the store of the record alone and X still advances.  (A batch
// never queues more steps than the log has slots, so the guard is never taken; samples the caller does not read in time are
// dropped, and counted, by the series on the host.)  A cancelled step (StepCtrl::active == 0) moves and records nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_kernels.h"      // StepCtrl, Half, Vec4, eos7
#include "sphmi_probes.h"       // ProbeSampleArgs, pr_walk
#include "sphmi_series.h"       // kMaxTracers, kTrParticleValues, kTrDrifterValues
#include "sphmi_step_record.h"  // StepRecord, the delivered row

namespace sphmi {

constexpr int kTrBlock = 256;
constexpr int kTrRecordMax = kStepHeader + (kTrParticleValues + kTrDrifterValues) * kMaxTracers;

template <class T> struct TracerParticleArgs {
    using V4 = typename Vec4<T>::type;
    StepRecord step;
    Half<const V4> pk0, pk1;             // the corrector's output set
    Half<const V4> half0;                // the half-step set: Pressure is Pressure!(ρₙ⁺), as k_pack_output delivers it
    const V4* comp;                      // fp32 handles: low words of position and density (null: none)
    const int* prow;                     // row at the last sphmi_download_permutation
    const int* slot_of_record;           // row of that epoch → slot of the tracked particle, −1: not tracked
    T rho0, inv_rho0, Cbe;
    int n_particles, N, D;
};

template <class T> struct TracerDrifterArgs {
    ProbeSampleArgs<T> s;                // the walk's arguments; pos: X (read and written), step: the tracers' log, n_probes: the drifters
    double* X;                           // 3 doubles per drifter (s.pos, writable)
    double min_weight;
    int value0;                          // first double of the drifters inside a record: kStepHeader + kTrParticleValues · n_particles
    int write_header;                    // no tracked particles: this kernel writes { iteration, time, Δt }
};

// enable: slot_of_record (all −1) gets the slot of every tracked row; rows[] are distinct and inside [0, n) (check_tracer_table)
__global__ void k_tr_map_init(const int* __restrict__ rows, const int* __restrict__ prow, int* __restrict__ slot_of_record, int n_particles, int n) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_particles) return;
    const unsigned r = (unsigned)rows[s];
    if (r >= (unsigned)n) return;
    const unsigned e = (unsigned)prow[r];
    if (e < (unsigned)n) slot_of_record[e] = s;
}

template <class T>
__global__ void __launch_bounds__(kTrBlock) k_tr_particles(const TracerParticleArgs<T> A) {
    using V4 = typename Vec4<T>::type;
    const StepCtrl c = *A.step.ctrl;
    if (!c.active) return;
    const long long slot = A.step.slot(c);
    if (slot < 0) return;
    double* rec = A.step.at(slot);
    const long long i = (long long)blockIdx.x * kTrBlock + (int)threadIdx.x;
    if (i == 0) A.step.write_header(rec, c);
    if (i >= (long long)A.N) return;
    const unsigned e = (unsigned)A.prow[i];
    if (e >= (unsigned)A.N) return;
    const unsigned s = (unsigned)A.slot_of_record[e];
    if (s >= (unsigned)A.n_particles) return;
    const V4 q0 = A.pk0[i], q1 = A.pk1[i];
    V4 lw; lw.x = lw.y = lw.z = lw.w = T(0);
    if (sizeof(T) == 4 && A.comp) lw = A.comp[i];
    double* v = rec + kStepHeader + (size_t)kTrParticleValues * s;
    v[0] = delivered_coord(q0.x, lw.x);
    v[1] = delivered_coord(q0.y, lw.y);
    v[2] = A.D == 3 ? delivered_coord(q0.z, lw.z) : 0.0;
    v[3] = (double)q1.x;
    v[4] = (double)q1.y;
    v[5] = A.D == 3 ? (double)q1.z : 0.0;
    v[6] = delivered_density(q0.w, lw.w);
    v[7] = (double)eos7<T>(A.half0[i].w, A.rho0, A.inv_rho0, A.Cbe);
}

template <class T>
__global__ void __launch_bounds__(256) k_tr_drift(const TracerDrifterArgs<T> A) {
    const StepCtrl c = *A.s.step.ctrl;
    if (!c.active) return;
    const long long slot = A.s.step.slot(c);
    const bool keep = slot >= 0;                                           // guards the record, not the walk: the move does not depend on the log
    const int lane = (int)threadIdx.x & 63;
    const int p = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    if (p >= A.s.n_probes) return;
    const double xp[3] = {A.X[3 * p], A.X[3 * p + 1], A.s.D == 3 ? A.X[3 * p + 2] : 0.0};
    PrSums sums;
    pr_walk<T>(A.s, xp, lane, sums);
    const double n = sums.n, S = sums.S, SP = sums.SP, Sr = sums.Sr, Sx = sums.Sx, Sy = sums.Sy, Sz = sums.Sz;
    if (lane != 0) return;
    if (S >= A.min_weight) {
#pragma clang fp contract(off)
        const double dt = c.last_dt;
        A.X[3 * p] = xp[0] + (Sx / S) * dt;
        A.X[3 * p + 1] = xp[1] + (Sy / S) * dt;
        if (A.s.D == 3) A.X[3 * p + 2] = xp[2] + (Sz / S) * dt;
    }
    if (!keep) return;
    double* rec = A.s.step.at(slot);
    if (p == 0 && A.write_header) A.s.step.write_header(rec, c);
    double* v = rec + A.value0 + (size_t)kTrDrifterValues * p;
    v[0] = xp[0]; v[1] = xp[1]; v[2] = xp[2];
    v[3] = S; v[4] = SP; v[5] = Sr; v[6] = Sx; v[7] = Sy; v[8] = A.s.D == 3 ? Sz : 0.0; v[9] = n;
}

}  // namespace sphmi
