// sphmi_maps.h — what every patch of the tank has experienced over time, accumulated on the device at every step (sphmi_maps_enable /
// _read / _disable): how high the water ever stood over each bin of a lattice, when it first got there, how long the bin stayed wet and
// the mean flow through it — crest, arrival time, wet duration, time-mean depth and velocity, the flood-map quantities.  The envelopes
// (sphmi_envelopes.h) are the Lagrangian record of a run at step resolution; this is the Eulerian one.  Nothing here is keyed by row:
// rebuilds, sphmi_download_permutation and attached columns are irrelevant by construction.
//
// The first part of this header is plain C++17 that also compiles as HIP (the index, the two integer images and the record arithmetic:
// tests/host_maps/maps_main.cpp calls them on a machine without a GPU); the kernels follow behind __HIPCC__.
//
// The lattice: bin (k0, k1, k2), index k0 + n0·(k1 + n1·k2) — the node order of sphmi_sample_grid — holds the rows with
//     k_d = floor((x_d − origin_d) / spacing_d),   0 <= k_d < counts_d   for every axis,
// x the fp64 Position fl_load forms (sphmi_flow.h; 2-D handles: z = 0 against origin 0, spacing +inf, count 1), one rounding for the
// subtraction, one for the division, compared as doubles BEFORE any conversion: a NaN falls outside.  An axis is collapsed by
// counts_d = 1, spacing_d = +inf: the same arithmetic yields ±0 for every finite coordinate, and 0 <= −0.  Only owned Fluid rows count,
// as fl_load recognises them, and of those only rows whose velocity is finite.
//
// Per executed step and bin, formed by k_mp_bin with order-independent integer operations only — every one exactly associative and
// commutative, so the bits do not depend on which lane, wave or workgroup got there first:
//     n        uint32   rows inside                                         atomic add
//     top      uint64   max of mp_image(x_up)                               atomic max      (identity 0)
//     bottom   uint64   min of mp_image(x_up)                               atomic min      (identity ~0)
//     S_d      int64    Σ llrint(v_d · 2³²), round to nearest even          atomic add      (2-D handles: S_2 stays an exact zero)
// mp_image is the order-preserving 64-bit integer image of a double (−0 < +0).  One unit of S is 2.3·10⁻¹⁰ m/s per row; with
// (rows of the handle) · max|v| < 2³¹ no sum overflows: the enable refuses handles with more than 2³¹ / (4·c₀) rows.
//
// The record of a bin, kMpValues doubles, one array per slot (slot · bins + bin).  With t = StepCtrl::total_time at the end of the step,
// dt = StepCtrl::last_dt, Sd_d = (double)S_d · 2⁻³² and u_d = Sd_d / (double)n, updated only when n > 0 — a dry bin is left alone:
//     slot  value                          start   update
//     0, 1  top_max, t_top_max             −inf, 0 if (top > top_max) { top_max = top; t_top_max = t; }
//     2     bottom_min                     +inf    if (bottom < bottom_min) bottom_min = bottom
//     3     t_arrival                      +inf    if (t_arrival == inf) t_arrival = t
//     4     wet = Σ dt                     0       wet = wet + dt
//     5     fill = Σ n·dt                  0       fill = fill + (double)n * dt
//     6–8   flux_d = Σ Sd_d·dt             0       flux_d = flux_d + Sd_d * dt
//     9, 10 speed2_max, t_speed2_max       0, 0    s = (ux*ux + uy*uy) + uz*uz; if (s > speed2_max) { speed2_max = s; t_speed2_max = t; }
//     11    n_max                          0       if ((double)n > n_max) n_max = (double)n
// Every operation is fp64, rounded once, contraction off (mp_fold): a host forms the same doubles from per-step downloads
// (sphexample_amd/maps.py: update).  There is no sqrt here.
//
// Two step buffers; the header { steps (int64 bits), t_begin, t_end, duration, seen (int64 bits) } lives on the device.  The step
// with `steps` executed steps before it uses buffer steps & 1, so a cancelled step needs no host knowledge:
//   k_mp_fill   enable: start records, both buffers at their identities, the header.
//   k_mp_bin    behind the corrector of every queued step, on its output set; returns at once when StepCtrl::active == 0.  One row
//               per lane.  Rows are in cell order, so neighbouring lanes mostly hit the same bin: a lane whose bin differs from its
//               lower neighbour's is the HEAD of a run (one __shfl_up, one __ballot), a segmented __shfl_down reduction in six steps
//               leaves the run's n / top / bottom / S in its head, and only heads of counting runs issue the 64-bit global atomics
//               — a wave without two equal neighbours skips the reduction.  The bin index is range-tested before the atomics and the
//               buffer is steps & 1.  Lane 0 of workgroup 0 notes `seen` = the steps it read: nobody writes `steps` in this launch.
//   k_mp_fold   one lane per bin: reads `seen` (nobody writes it in this launch), clears the OTHER buffer's wet bins — the map of
//               the step before, which the next step will fill again — then reads the count ALONE for a dry bin and folds a wet one
//               with mp_fold: every record has one writer, no atomics.  Lane 0 of workgroup 0 moves the window on.
// The buffer of the last executed step stays as it is until the step after the next: sphmi_maps_read delivers it as the instantaneous
// map (n, top, bottom, Sd), without a Shepard sum.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "sphmi_series.h"       // kMpValues, kMpHeader

#ifndef SPHMI_HD
#if defined(__HIPCC__)
#define SPHMI_HD __host__ __device__ inline
#else
#define SPHMI_HD inline
#endif
#endif
#ifndef SPHMI_NO_CONTRACT
#if defined(__clang__)
#define SPHMI_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SPHMI_NO_CONTRACT                        /* (the host program is compiled with -ffp-contract=off) */
#endif
#endif

namespace sphmi {

constexpr int kMpHeaderDev = kMpHeader + 2;      // … + `seen`, the step count k_mp_bin read (int64 bits), and 8 bytes that keep what follows on 16

// the lattice as the kernels see it: three axes (2-D handles: the third is origin 0, spacing +inf, count 1)
struct MapLattice {
    double origin[3], spacing[3], countd[3];     // countd = (double)counts
    int counts[3];
    int up, bins;
};

// the order-preserving integer image of a double: a < b  ⇔  mp_image(a) < mp_image(b) as unsigned, −0 below +0
SPHMI_HD uint64_t mp_image(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
SPHMI_HD double mp_value(uint64_t u) {
    const uint64_t b = (u >> 63) ? u & 0x7fffffffffffffffull : ~u;
    double v;
    memcpy(&v, &b, 8);
    return v;
}
constexpr uint64_t kMpTopIdentity = 0ull, kMpBottomIdentity = ~0ull;

// a velocity component in units of 2⁻³² m/s, round to nearest even (the product by a power of two is exact)
SPHMI_HD long long mp_fixed(double v) { return llrint(v * 4294967296.0); }
SPHMI_HD double mp_unfixed(long long S) { return (double)S * (1.0 / 4294967296.0); }
SPHMI_HD bool mp_finite(double v) { return fabs(v) < (double)INFINITY; }

// the bin of a position, −1 outside the lattice
SPHMI_HD int mp_bin(const MapLattice& L, double x, double y, double z) {
    SPHMI_NO_CONTRACT
    const double k0 = floor((x - L.origin[0]) / L.spacing[0]);
    const double k1 = floor((y - L.origin[1]) / L.spacing[1]);
    const double k2 = floor((z - L.origin[2]) / L.spacing[2]);
    if (!(k0 >= 0.0 && k0 < L.countd[0] && k1 >= 0.0 && k1 < L.countd[1] && k2 >= 0.0 && k2 < L.countd[2])) return -1;
    return (int)k0 + L.counts[0] * ((int)k1 + L.counts[1] * (int)k2);
}

// the start record of slot `slot`
SPHMI_HD double mp_start(int slot) { return slot == 0 ? -(double)INFINITY : (slot == 2 || slot == 3) ? (double)INFINITY : 0.0; }

// one executed step of a WET bin (n > 0): r[slot · stride] is slot `slot` of its record
SPHMI_HD void mp_fold(double* r, size_t stride, uint32_t n, uint64_t top_image, uint64_t bottom_image, const long long* S, double t, double dt) {
    SPHMI_NO_CONTRACT
    const double inf = (double)INFINITY;
    const double top = mp_value(top_image), bottom = mp_value(bottom_image), nd = (double)n;
    if (top > r[0]) { r[0] = top; r[stride] = t; }
    if (bottom < r[2 * stride]) r[2 * stride] = bottom;
    if (r[3 * stride] == inf) r[3 * stride] = t;
    r[4 * stride] = r[4 * stride] + dt;
    r[5 * stride] = r[5 * stride] + nd * dt;
    const double sx = mp_unfixed(S[0]), sy = mp_unfixed(S[1]), sz = mp_unfixed(S[2]);
    r[6 * stride] = r[6 * stride] + sx * dt;
    r[7 * stride] = r[7 * stride] + sy * dt;
    r[8 * stride] = r[8 * stride] + sz * dt;
    const double ux = sx / nd, uy = sy / nd, uz = sz / nd;
    const double s = (ux * ux + uy * uy) + uz * uz;
    if (s > r[9 * stride]) { r[9 * stride] = s; r[10 * stride] = t; }
    if (nd > r[11 * stride]) r[11 * stride] = nd;
}

}  // namespace sphmi

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "sphmi_flow.h"         // fl_load: the owned Fluid rows and their fp64 position
#include "sphmi_kernels.h"      // StepCtrl, Half, Vec4

namespace sphmi {

constexpr int kMpBlock = 256;

// the memory of an enabled handle: the records, the two step buffers, the header
struct MapStore {
    double* record;                      // kMpValues arrays of `bins` doubles
    unsigned long long* step64[2];       // per buffer five arrays of `bins` words: top, bottom (images), S_0, S_1, S_2 (int64 bits)
    unsigned* count[2];                  // per buffer `bins` counts
    double* header;                      // kMpHeaderDev doubles
};

template <class T> struct MapArgs {
    using V4 = typename Vec4<T>::type;
    const StepCtrl* ctrl;                // the block this step's corrector read
    Half<const V4> pk0, pk1;             // the corrector's output set
    const V4* comp;                      // fp32 handles: low words of position and density (null: none)
    const uint8_t* type;                 // always null here (single-device handles): Fluid off the sign of the ρ·s slot, as fl_load reads it
    MapStore m;
    MapLattice lat;
    int N, D;
};

__global__ void __launch_bounds__(kMpBlock) k_mp_fill(const MapStore m, int bins, double t_begin) {
    const int b = blockIdx.x * kMpBlock + (int)threadIdx.x;
    if (b == 0) {
        m.header[0] = __longlong_as_double(0ll); m.header[1] = t_begin; m.header[2] = t_begin; m.header[3] = 0.0;
        m.header[4] = __longlong_as_double(0ll); m.header[5] = 0.0;
    }
    if (b >= bins) return;
#pragma unroll
    for (int s = 0; s < kMpValues; ++s) m.record[(size_t)s * bins + b] = mp_start(s);
    for (int p = 0; p < 2; ++p) {
        m.count[p][b] = 0u;
        m.step64[p][b] = kMpTopIdentity;
        m.step64[p][(size_t)bins + b] = kMpBottomIdentity;
        for (int d = 0; d < 3; ++d) m.step64[p][(size_t)(2 + d) * bins + b] = 0ull;
    }
}

template <class T>
__global__ void __launch_bounds__(kMpBlock) k_mp_bin(const MapArgs<T> A) {
#pragma clang fp contract(off)
    if (!A.ctrl->active) return;
    const long long steps = __double_as_longlong(A.m.header[0]);
    const int p = (int)(steps & 1ll);
    const long long i = (long long)blockIdx.x * kMpBlock + (int)threadIdx.x;
    if (i == 0) A.m.header[4] = __longlong_as_double(steps);
    const FlowRow<T> r = fl_load<T>(A, i, true);
    int bin = -1;
    if (r.counts && mp_finite(r.vx) && mp_finite(r.vy) && mp_finite(r.vz)) bin = mp_bin(A.lat, r.x, r.y, r.z);
    const bool in = bin >= 0;
    const double up = A.lat.up == 0 ? r.x : A.lat.up == 1 ? r.y : r.z;
    unsigned n = in ? 1u : 0u;
    unsigned long long top = in ? mp_image(up) : kMpTopIdentity, bottom = in ? mp_image(up) : kMpBottomIdentity;
    long long sx = in ? mp_fixed(r.vx) : 0ll, sy = in ? mp_fixed(r.vy) : 0ll, sz = in ? mp_fixed(r.vz) : 0ll;

    // runs of equal bin inside the wave: the head of a run collects it
    const int lane = (int)threadIdx.x & 63;
    const int below = __shfl_up(bin, 1, 64);
    const bool head = lane == 0 || below != bin;
    const unsigned long long heads = __ballot(head);
    if (heads != ~0ull) {                // (wave-uniform)
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        const int end = above ? lane + (int)__ffsll((long long)above) : 64;        // the first lane behind this lane's run
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned on = __shfl_down(n, d, 64);
            const unsigned long long ot = __shfl_down(top, d, 64), ob = __shfl_down(bottom, d, 64);
            const long long ox = __shfl_down(sx, d, 64), oy = __shfl_down(sy, d, 64), oz = __shfl_down(sz, d, 64);
            if (lane + d < end) {
                n += on;
                top = ot > top ? ot : top; bottom = ob < bottom ? ob : bottom;
                sx += ox; sy += oy; sz += oz;
            }
        }
    }
    if (!head || !in || (unsigned)bin >= (unsigned)A.lat.bins) return;
    const size_t bins = (size_t)A.lat.bins;
    unsigned long long* w = A.m.step64[p] + bin;
    atomicAdd(A.m.count[p] + bin, n);
    atomicMax(w, top);
    atomicMin(w + bins, bottom);
    atomicAdd(w + 2 * bins, (unsigned long long)sx);
    atomicAdd(w + 3 * bins, (unsigned long long)sy);
    if (A.D == 3) atomicAdd(w + 4 * bins, (unsigned long long)sz);
}

__global__ void __launch_bounds__(kMpBlock) k_mp_fold(const StepCtrl* __restrict__ ctrl, const MapStore m, int bins) {
    if (!ctrl->active) return;
    const double t = ctrl->total_time, dt = ctrl->last_dt;
    const long long steps = __double_as_longlong(m.header[4]);
    const int p = (int)(steps & 1ll);
    const int b = blockIdx.x * kMpBlock + (int)threadIdx.x;
    if (b == 0) {
        // the window: one lane of the launch (the launches of a stream run in step order)
        m.header[0] = __longlong_as_double(steps + 1ll);
        m.header[2] = t;
        m.header[3] = m.header[3] + dt;
    }
    if (b >= bins) return;
    const size_t B = (size_t)bins;
    if (m.count[p ^ 1][b]) {             // the map of the step before: the next step starts from the identities
        unsigned long long* o = m.step64[p ^ 1] + b;
        m.count[p ^ 1][b] = 0u;
        o[0] = kMpTopIdentity; o[B] = kMpBottomIdentity; o[2 * B] = 0ull; o[3 * B] = 0ull; o[4 * B] = 0ull;
    }
    const unsigned n = m.count[p][b];
    if (!n) return;                      // a dry bin: the count alone was read
    const unsigned long long* w = m.step64[p] + b;
    const long long S[3] = {(long long)w[2 * B], (long long)w[3 * B], (long long)w[4 * B]};
    mp_fold(m.record + b, B, n, w[0], w[B], S, t, dt);
}

}  // namespace sphmi
#endif
