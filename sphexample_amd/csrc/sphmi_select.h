// sphmi_select.h — a selected subset of the rows, compacted on the device on demand (sphmi_select_build / _read / _download* / _release).
//
// A row is SELECTED iff every enabled clause of the selection holds (the clauses are ANDed, the boxes of the spatial clause ORed):
//   type     bit (Type − 1) of type_mask is set — always on
//   boxes    lo[b][d] <= x[d] < hi[b][d] for every d < dims, for SOME box b — the half-open test of sphmi_flow.h, ±inf allowed
//   markers  GroupMarker is one of markers[]
//   id       (uint64)ID % id_stride == id_phase — keyed on the particle, not on the row: the same particles through every sort
//   field    field_lo <= value <= field_hi, value the Density, the Pressure or SPEED2 = (vx·vx + vy·vy) + vz·vz; a NaN is never kept
//   mask     the caller's byte of the row is non-zero
// on the doubles a handle with Float64 host arrays would deliver for the row NOW, formed as k_pack_output forms them (Position and
// Density: record + low word on fp32 handles, the sign of ρ stripped; Pressure: Pressure!(ρₙ⁺) of the half-step set after the first
// step, the record's before it), every operation rounded once: sel_keep and sel_speed2 below are compiled with contraction off, by
// the device AND by the stand-alone host program of tests/host_select — a host reproduces the selection bit for bit from a download.
//
// Four kernels, all on the engine's stream:
//   k_sel_flag        one row per lane → an int flag.  A streaming pass: it loads the type byte always and, behind branches on the kernel
//                     arguments (uniform: no lane decides), only the columns the enabled clauses read — pk0 (+ the low words) with boxes
//                     or DENSITY, pk1 / the half-step pk0 with SPEED2 / PRESSURE, id with a stride > 1, grp with markers, the mask byte
//                     with a mask.  Bytes per row: 1 + 4 (the flag) + 2·sizeof(V4) per packet touched (the interleaved record's line
//                     carries both packets) + sizeof(V4) low words + 8 + 8 + 1.
//   scan64            (sphmi_results.h) flags → int64 offsets, offsets[N] = n_selected
//   k_sel_fill        rows[offsets[i]] = i for every flagged i: ascending, no atomic decides a place — repeated builds give the same bytes
//   k_pack_selected   slot s < n_selected packs row rows[s] with pack_output_row, the per-row body of k_pack_output (sphmi_rebuild.h), and
//                     gathers ID, Type and GroupMarker.  The columns go through k_gather_selected_columns (sphmi_columns.h).
// The box and marker tables travel by value in the kernel arguments (SelSpec, 1 KiB).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
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

// ---- the plain C++ part: what tests/host_select/select_main.cpp compiles ------------------------------------------------------------
constexpr int kSelMaxBoxes = 16, kSelMaxMarkers = 16;
enum { kSelFieldNone = 0, kSelFieldDensity = 1, kSelFieldPressure = 2, kSelFieldSpeed2 = 3 };

// by value in the kernel arguments
struct SelSpec {
    uint32_t type_mask;                  // bit (Type − 1)
    int32_t n_boxes, n_markers, field, dims, has_mask;
    int64_t id_stride, id_phase;         // 1 <= stride, 0 <= phase < stride
    double field_lo, field_hi;
    double lo[kSelMaxBoxes][3], hi[kSelMaxBoxes][3];
    uint64_t markers[kSelMaxMarkers];
};

// what the clauses read of a row; members of a clause that is off are never looked at
struct SelRow {
    int32_t type;
    double x[3];
    double value;                        // of SelSpec::field
    int64_t id;
    uint64_t group;
    uint8_t mask;
};

// one rounding per operation, never contracted
SPHMI_HD double sel_speed2(double vx, double vy, double vz) {
    SPHMI_NO_CONTRACT
    return (vx * vx + vy * vy) + vz * vz;
}

SPHMI_HD bool sel_keep(const SelSpec& s, const SelRow& r) {
    SPHMI_NO_CONTRACT
    if (r.type < 1 || r.type > 3 || !((s.type_mask >> (r.type - 1)) & 1u)) return false;
    if (s.n_boxes > 0) {
        bool any = false;
        for (int b = 0; b < s.n_boxes; ++b) {
            // (the axes written out: r.x is never indexed by a run-time value, so it stays in registers on the device)
            const bool in = s.lo[b][0] <= r.x[0] && r.x[0] < s.hi[b][0] && s.lo[b][1] <= r.x[1] && r.x[1] < s.hi[b][1] &&
                            (s.dims < 3 || (s.lo[b][2] <= r.x[2] && r.x[2] < s.hi[b][2]));
            any = any || in;
        }
        if (!any) return false;
    }
    if (s.n_markers > 0) {
        bool any = false;
        for (int k = 0; k < s.n_markers; ++k) any = any || r.group == s.markers[k];
        if (!any) return false;
    }
    if (s.id_stride > 1 && (uint64_t)r.id % (uint64_t)s.id_stride != (uint64_t)s.id_phase) return false;
    if (s.field != kSelFieldNone && !(s.field_lo <= r.value && r.value <= s.field_hi)) return false;      // (a NaN value fails both)
    if (s.has_mask && r.mask == 0) return false;
    return true;
}

}  // namespace sphmi

// ---- the device part ------------------------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "sphmi_kernels.h"
#include "sphmi_rebuild.h"

namespace sphmi {

constexpr int kSelThreads = 256;

template <class T> struct SelFlagArgs {
    using V4 = typename Vec4<T>::type;
    Half<const V4> pk0, pk1, half0;      // the set sphmi_download reads; half0: null before the first step
    const V4* comp;                      // fp32 handles: the low words (null: none)
    const uint8_t* type;
    const long long* id;
    const unsigned long long* grp;
    const uint8_t* mask;                 // the caller's bytes on the device (null: no mask clause)
    int* flags;                          // [N]
    int N;
    T rho0, inv_rho0, Cbe;
};

template <class T>
__global__ void __launch_bounds__(kSelThreads) k_sel_flag(const SelFlagArgs<T> A, const SelSpec S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.N) return;
    SelRow r;
    r.type = (int32_t)A.type[i];
    r.x[0] = r.x[1] = r.x[2] = 0.0; r.value = 0.0; r.id = 0; r.group = 0; r.mask = 0;
    // (every branch below tests kernel arguments only: the wave takes it or skips it as one)
    if (S.n_boxes > 0 || S.field == kSelFieldDensity) {
        const auto q = A.pk0[i];
        double rho = (double)(q.w < T(0) ? -q.w : q.w);
        r.x[0] = (double)q.x; r.x[1] = (double)q.y; r.x[2] = (double)q.z;
        if (sizeof(T) == 4 && A.comp) {
            const auto c = A.comp[i];
            r.x[0] += (double)c.x; r.x[1] += (double)c.y; r.x[2] += (double)c.z; rho += (double)c.w;
        }
        if (S.field == kSelFieldDensity) r.value = rho;
    }
    if (S.field == kSelFieldSpeed2 || (S.field == kSelFieldPressure && !A.half0)) {
        const auto q = A.pk1[i];
        if (S.field == kSelFieldSpeed2) r.value = sel_speed2((double)q.x, (double)q.y, S.dims == 3 ? (double)q.z : 0.0);
        else r.value = (double)q.w;
    }
    if (S.field == kSelFieldPressure && A.half0) r.value = (double)eos7<T>(A.half0[i].w, A.rho0, A.inv_rho0, A.Cbe);
    if (S.id_stride > 1) r.id = A.id[i];
    if (S.n_markers > 0) r.group = A.grp[i];
    if (S.has_mask) r.mask = A.mask[i];
    A.flags[i] = sel_keep(S, r) ? 1 : 0;
}

// offsets: the exclusive scan of flags, offsets[N] = n_sel
__global__ void __launch_bounds__(kSelThreads) k_sel_fill(const int* __restrict__ flags, const long long* __restrict__ offsets, int N, long long n_sel,
                                                          int* __restrict__ rows) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || !flags[i]) return;
    const long long o = offsets[i];
    if (o >= 0 && o < n_sel) rows[o] = i;                    // (the scan makes it so: the test keeps a damaged offset from becoming a wild store)
}

// ID, Type and GroupMarker of the selected rows: sphmi_download copies the whole columns, a selection gathers them
struct SelTags {
    const long long* id; const uint8_t* type; const unsigned long long* grp;
    long long* id_out; uint8_t* type_out; unsigned long long* grp_out;      // [n_sel] each (null = not requested)
};

template <class T, class H>
__global__ void __launch_bounds__(kSelThreads) k_pack_selected(const int* __restrict__ rows, int n_sel,
                                                               Half<const typename Vec4<T>::type> pk0, Half<const typename Vec4<T>::type> pk1,
                                                               Half<const typename Vec4<T>::type> half0, const typename Vec4<T>::type* accv,
                                                               const typename Vec4<T>::type* ghostv, const typename Vec4<T>::type* comp,
                                                               const int* key, int N, int D, int C,
                                                               GridDesc g, int have_grid, T rho0, T inv_rho0, T Cbe, OutFields<H> o, SelTags t) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_sel) return;
    const int i = rows[s];
    if ((unsigned)i >= (unsigned)N) return;                  // (cannot happen: k_sel_fill wrote a row index)
    pack_output_row<T, H>(i, (size_t)s, pk0, pk1, half0, accv, ghostv, comp, key, D, C, g, have_grid, rho0, inv_rho0, Cbe, o);
    if (t.id_out) t.id_out[s] = t.id[i];
    if (t.type_out) t.type_out[s] = t.type[i];
    if (t.grp_out) t.grp_out[s] = t.grp[i];
}

}  // namespace sphmi
#endif
