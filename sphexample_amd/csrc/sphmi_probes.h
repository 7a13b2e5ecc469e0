// sphmi_probes.h — pressure, density and velocity sampled at fixed probe points on every step (sphmi_probes_enable / _read).
//
// For every EXECUTED step and every probe p at the fixed position x_p, over the rows j the handle owns with Type == Fluid and
// |x_p − x_j|² ≤ H² (the reference's inclusive cut, src/SPHCellList.jl:275, on the CURRENT positions):
//     w_j = (m₀ / ρ_j) · W(|x_p − x_j|)          W: the handle's kernel (src/SPHKernels.jl:75-91), its αD and h
//     n = rows      S = Σ w_j      SP = Σ w_j P_j      Sρ = Σ w_j ρ_j      Sv = Σ w_j v_j
// on the state sphmi_download would deliver directly after that step: Position, Density (fp32 handles: record + low word),
// Velocity of the corrector's output set, Pressure = Pressure!(ρₙ⁺) of the half-step set, evaluated with the arithmetic of
// k_pack_output.  A probe is not a particle: no self term, r = 0 is legal.  Everything is summed in fp64, on fp32 handles too.
// The RAW sums are recorded; the host normalises at read time (a multi-device handle adds the slabs' sums first).
//
// k_probe_sample — one wave per probe, queued behind every corrector (Engine::pr_sample), like k_gf_* (sphmi_group_forces.h):
// returns at once when the step was cancelled, writes this step's record of the batch's log (StepRecord, sphmi_step_record.h).
//
// EXACT, NOT STALE.  The pair loop reproduces the reference's stale cell lists (quirk Q1); a probe has no such quirk to keep.  The rows
// are still found through `cstart`, i.e. through the cell every row was hashed into at the last rebuild, so the candidate cells
// must cover how far a row may have drifted since:
//   * a cell is where map_floor rounds to: row j of cell c had |x_j / H − c| ≤ ½ per axis at the rebuild;
//   * every step's control adds 4 · max_i |Positionₙ⁺ − Position| of the step before to Δx and asks for the rebuild at Δx ≥ h
//     (src/SPHCellList.jl:706-724, 744, 758).  That difference is (v − vₙ/2)·Δt, half the step's displacement v·Δt up to the
//     change of velocity within the step: a row moves ≤ 2·max|…| + |a|Δt²/2 per step, and Δt ≤ CFL·√(h/|a|max) bounds the
//     last term by CFL²·h/2.  While steps execute Δx < h, so the steps BEFORE the sampled one moved a row by less than
//     2·h/4 = h/2 (+ the small acceleration terms); the sampled step itself, which no control has counted yet, by |v|Δt ≤
//     CFL·h·|v|/c₀ — a few per cent of h in a weakly compressible run;
//   * margin = h: twice the h/2 of the counted steps.  The candidate cells of a probe are all cells c with
//     [c − ½, c + ½] ∩ [(x_p − H − h)/H, (x_p + H + h)/H] ≠ ∅ per axis — up to FOUR per axis at H = 2h (five for k < 2), not
//     three — widened by 1e-6 relative for the fp32 rounding of map_floor; the exact cut r² ≤ H² is applied per candidate in fp64.
//   (tests/test_probes_gpu.py::test_stale_lists checks steps far behind a rebuild against an O(M·N) enumeration.)
//
// For every (cy, cz) the x-adjacent candidate cells are ONE index range of the sorted rows.  The ranges are cut into jobs of 64
// consecutive rows, numbered in (cz, cy, row) order; the wave takes the jobs in that order, lane l row l of each, four jobs'
// loads in flight (both 16-byte packets of a record, the half-step density, fp32: the low words).  Every lane adds its rows
// in job order, then one fixed butterfly over the lanes: the order of every sum is a function of the row order alone — no
// atomics — and repeated runs give the same bits.  Grid origin and extent, `cstart` and the record sets are those of the
// corrector queued in front (by value, taken at queue time like ForceParams / MdbcParams: rebuilds — device-side ones
// included — are queued between batches and keep the grid of a handle that rebuilds on the device).
// A probe outside the dense grid clamps to empty ranges: S = 0, n = 0.  Dead rows and ghost copies of a slab handle (type byte)
// are skipped; plain handles read Fluid off the sign of the ρ·s slot.
//
// Record (kStepHeader + kPrValues · n_probes doubles): the header, then { S, SP, Sρ, Sv[0..2], n }[p]; 2-D handles write a zero third
// velocity component.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_kernels.h"
#include "sphmi_rebuild.h"
#include "sphmi_series.h"       // kMaxProbes, kPrValues
#include "sphmi_step_record.h"  // StepRecord, wave_sum

namespace sphmi {

constexpr int kPrRecordMax = kStepHeader + kPrValues * kMaxProbes;
constexpr int kPrMaxRows = 25;           // (cy, cz) pairs of a probe: ≤ 5 × 5 — H + h ≤ 2H spans at most five cells per axis
constexpr int kPrInFlight = 4;           // jobs whose loads are issued before the first is used

template <class T> struct ProbeSampleArgs {
    using V4 = typename Vec4<T>::type;
    StepRecord step;
    Half<const V4> pk0, pk1;             // the corrector's output set
    Half<const V4> half0;                // the half-step set: Pressure!(ρₙ⁺), src/SPHCellList.jl:789
    const V4* comp;                      // fp32 handles: low words of position and density (null: none)
    const uint8_t* type;                 // slab handles: the type byte (ghost copies, dead rows); null on plain handles
    const int* cstart;
    const double* pos;                   // 3 doubles per probe
    GridDesc g;
    double H_inv, H2, h_inv, reach;      // reach = H + margin (above)
    double alphaD, m0;
    T rho0, inv_rho0, Cbe;
    int n_probes, N, D, kernel;
};

// W(q) of src/SPHKernels.jl:75-78 (Wendland C2) and :89-92 (CubicSpline), fp64
__device__ __forceinline__ double pr_kernel_w(int kernel, double alphaD, double q) {
    if (kernel == 1) {                   // SPHMI_KERNEL_CUBIC_SPLINE
        const double a = q <= 1.0 ? 1.0 - 1.5 * q * q + 0.75 * q * q * q : 0.0;
        const double t = 2.0 - q;
        const double b = (q > 1.0 && q <= 2.0) ? 0.25 * t * t * t : 0.0;
        return alphaD * (a + b);
    }
    const double t = 1.0 - 0.5 * q, t2 = t * t;
    return alphaD * (t2 * t2) * (2.0 * q + 1.0);
}

// The seven sums of a probe, as one lane carries them through the walk.  `add` is handed one accepted row — its weight w, Pressure, density,
// velocity and d = x_p − x_j — and `reduce` closes the walk with one fixed butterfly per sum.  pr_walk is written over such a set:
// PmSums (sphmi_probe_moments.h) carries these seven, formed by these statements, and the moment sums behind them.
struct PrSums {
    static constexpr int kInFlight = kPrInFlight;
    double n = 0.0, S = 0.0, SP = 0.0, Sr = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0;
    __device__ __forceinline__ void add(double w, double P, double rho, double vx, double vy, double vz, double, double, double) {
#pragma clang fp contract(off)
        n += 1.0; S += w; SP += w * P; Sr += w * rho;
        Sx += w * vx; Sy += w * vy; Sz += w * vz;
    }
    __device__ __forceinline__ void reduce() {
        n = wave_sum(n); S = wave_sum(S); SP = wave_sum(SP); Sr = wave_sum(Sr);
        Sx = wave_sum(Sx); Sy = wave_sum(Sy); Sz = wave_sum(Sz);
    }
};

// The walk of one wave over the candidate rows of the point xp (the header comment): the sums of `s` (zero on entry), complete in every
// lane.  `A` supplies the record sets, the cell list and the constants; its point table and its log are not touched.  `Sums` names the
// per-row statements and how many jobs' loads are in flight (kInFlight).  k_probe_sample, the drifters of sphmi_tracers.h and
// k_probe_moments (sphmi_probe_moments.h) call it: a moving point is sampled with the arithmetic, and in the order, of a fixed one.
template <class T, class Sums>
__device__ __forceinline__ void pr_walk(const ProbeSampleArgs<T>& A, const double (&xp)[3], const int lane, Sums& s) {
    constexpr int kInFlight = Sums::kInFlight;
    using V4 = typename Vec4<T>::type;
    // padded cell range per axis, clamped to the grid (in fp64 before the conversion: a probe may be anywhere)
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool empty = false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        if (d >= A.D) continue;
        double a = (xp[d] - A.reach) * A.H_inv, b = (xp[d] + A.reach) * A.H_inv;
        a -= 1e-6 * (1.0 + fabs(a)); b += 1e-6 * (1.0 + fabs(b));
        const double off = 1.0 - (double)A.g.gmin[d], top = (double)(A.g.np[d] - 1);
        const double l = fmax(ceil(a - 0.5) + off, 0.0), u = fmin(floor(b + 0.5) + off, top);
        if (!(l <= u)) empty = true;                        // outside the grid (a NaN coordinate cannot get here: sphmi_probes_enable refuses it)
        lo[d] = empty ? 0 : (int)l; hi[d] = empty ? 0 : (int)u;
    }
    const int ny = hi[1] - lo[1] + 1, nz = A.D == 3 ? hi[2] - lo[2] + 1 : 1;
    const int nrow = empty ? 0 : min(ny * nz, kPrMaxRows);
    // row r = (cy, cz): its x-adjacent cells are one range of rows (lane r < nrow)
    int rs = 0, rc = 0;
    if (lane < nrow) {
        const int cy = lo[1] + lane % ny, cz = A.D == 3 ? lo[2] + lane / ny : 0;
        const int row = A.g.np[0] * (cy + A.g.np[1] * cz);
        rs = A.cstart[row + lo[0]];
        rc = A.cstart[row + hi[0] + 1] - rs;
        if (rs < 0 || rc < 0 || rs + rc > A.N) { rs = 0; rc = 0; }      // (cannot happen on a consistent cell list; keeps every load inside the arrays)
    }
    // jobs of 64 rows, numbered through the ranges: range r holds jobs [jexcl(r), jincl(r))
    int jincl = (rc + 63) >> 6;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) { const int u = __shfl_up(jincl, o, 64); if (lane >= o) jincl += u; }
    const int jexcl = jincl - ((rc + 63) >> 6);
    const int njobs = nrow > 0 ? __shfl(jincl, nrow - 1, 64) : 0;
    for (int jbase = 0; jbase < njobs; jbase += 64) {
        // lane l describes job jbase + l: its first row and the rows left in its range
        int job_first = 0, job_left = 0;
        {
            const int jb = jbase + lane;
            for (int r = 0; r < nrow; ++r) {
                const int e = __shfl(jexcl, r, 64), st = __shfl(rs, r, 64), cn = __shfl(rc, r, 64);
                const int o = (jb - e) << 6;
                if (jb >= e && o < cn) { job_first = st + o; job_left = cn - o; }
            }
        }
        const int nj = min(64, njobs - jbase);
        for (int j0 = 0; j0 < nj; j0 += kInFlight) {
            V4 q0[kInFlight], q1[kInFlight], lw[kInFlight];
            T hw[kInFlight];
            uint8_t ty[kInFlight];
            bool ok[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) {
                const int jl = min(j0 + u, 63);
                const int first = __shfl(job_first, jl, 64), left = j0 + u < nj ? __shfl(job_left, jl, 64) : 0;
                ok[u] = lane < left;
                const int k = ok[u] ? first + lane : 0;
                q0[u] = A.pk0[k]; q1[u] = A.pk1[k]; hw[u] = A.half0[k].w;
                if (sizeof(T) == 4 && A.comp) lw[u] = A.comp[k]; else { lw[u].x = lw[u].y = lw[u].z = lw[u].w = T(0); }
                ty[u] = A.type ? A.type[k] : (uint8_t)(q0[u].w > T(0) ? 1 : 2);
            }
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) {
                // (no contraction: r² is ((dx² + dy²) + dz²) rounded term by term, the value a host reference forms from the downloaded positions —
                // a row AT the cut is in or out for both)
#pragma clang fp contract(off)
                const bool fluid = (ty[u] & kTypeMask) == 1 && !(ty[u] & kGhostMask);       // SPHMI_FLUID, owned
                const double dx = xp[0] - ((double)q0[u].x + (double)lw[u].x), dy = xp[1] - ((double)q0[u].y + (double)lw[u].y),
                             dz = A.D == 3 ? xp[2] - ((double)q0[u].z + (double)lw[u].z) : 0.0;
                const double r2 = dx * dx + dy * dy + dz * dz;
                if (ok[u] && fluid && r2 <= A.H2) {
                    const double rho = (double)(q0[u].w < T(0) ? -q0[u].w : q0[u].w) + (double)lw[u].w;
                    // Pressure as k_pack_output delivers it: Pressure!(ρₙ⁺) in the handle's arithmetic
                    const T rr = sizeof(T) == 8 ? hw[u] / A.rho0 : hw[u] * A.inv_rho0;
                    const T rr2 = rr * rr, rr4 = rr2 * rr2;
                    const double P = (double)(A.Cbe * (rr4 * rr2 * rr - T(1)));
                    const double w = (A.m0 / rho) * pr_kernel_w(A.kernel, A.alphaD, sqrt(r2) * A.h_inv);
                    s.add(w, P, rho, (double)q1[u].x, (double)q1[u].y, (double)q1[u].z, dx, dy, dz);
                }
            }
        }
    }
    s.reduce();
}

template <class T>
__global__ void __launch_bounds__(256) k_probe_sample(const ProbeSampleArgs<T> A) {
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
    PrSums s;
    pr_walk<T>(A, xp, lane, s);
    if (lane == 0) {
        double* v = rec + kStepHeader + (size_t)kPrValues * p;
        v[0] = s.S; v[1] = s.SP; v[2] = s.Sr; v[3] = s.Sx; v[4] = s.Sy; v[5] = A.D == 3 ? s.Sz : 0.0; v[6] = s.n;
    }
}

}  // namespace sphmi
