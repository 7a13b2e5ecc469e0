// sphmi_rays.h — WHERE along a line does the water begin: the first crossing of S = level along up to 2²⁰ rays, on demand
// (sphmi_cast_rays).  A gauge, the run-up along a slope, the wetted height on an obstacle, the depth image a viewer renders from.
//
// At the parameter t of a ray the point is x[a] = o[a] + t · d[a] (one multiply, one add, not contracted) and the kernel forms the
// sums of k_point_cloud / k_point_gradients at x — n, S, SP, Sρ, Sv over the rows j the handle owns with Type == Fluid and
// r² = ((dx² + dy²) + dz²) ≤ H² on the state sphmi_download would deliver now, fp64, ascending row order, no self term, no atomics,
// no cross-lane reduction inside a sum.  inside(t) is S(t) ≥ level; a point outside the cell grid reads zeros and is outside.
//
// MARCH.  K = ⌈(t_end − t_begin) / step⌉ intervals (the host, fp64), t_k = t_begin + k · step for k < K, t_K = t_end exactly.  The
// crossing is the smallest k in 1 … K whose ends disagree the way `mode` asks (ENTER: out → in, LEAVE: in → out, ANY: either).
// REFINEMENT.  From (a, b) = (t_{k−1}, t_k), kRayRefineRounds rounds: δ = (b − a) / 64, u_m = a + m · δ for m = 1 … 63, u_0 = a,
// u_64 = b; the new bracket is (u_{m−1}, u_m) for the smallest m whose side differs from the side of a (m = 64 if none of
// u_1 … u_63 does: b differs by construction).  A round with δ == 0 leaves the bracket.  Four rounds narrow the interval by 2²⁴.
// The record — point and the five sums — is that of the INSIDE end of the final bracket: b for an entering crossing, a for a
// leaving one, so that it always describes fluid, S ≥ level.
//
// k_cast_rays — ONE WAVE PER RAY, no LDS.  A march round evaluates 64 consecutive march points, one per lane; every lane walks
// the candidate cells of its OWN point — the span of k_point_cloud for a tile of one point: the cells within H + h per axis, the
// probes' 1e-6, clamped to the grid, ≤ 4^D cells at H = 2h and 5^D for k < 2 — in (cz, cy, row) order, which is ascending row
// order, two rows' loads in flight, the conversions of k_point_cloud's staging and its statements for the cut and the sums.  The
// converted values pass an empty asm, as they pass LDS there: the compiler fuses multiply-adds in the sums as it does in that kernel,
// and the bits are those of sphmi_sample_point_gradients at the same point (tests/test_rays_gpu.py checks this bitwise against a
// host that restates the search with that call as its only evaluator).  A lane takes the side of k − 1 from the lane below, lane 0
// from the round before; a ballot and a find-first give the crossing, and the wave leaves the march at the first round that holds
// one.  A refinement round is the same evaluation at u_1 … u_63 in lanes 1 … 63.  The lane that evaluates the inside end of a
// new bracket keeps its sums; an inside end that survives from the march is evaluated once more by lane 0.  Neighbouring march
// points share most candidate cells: the lanes of a wave read the same rows, from L1 / L2 (profiles/rays.md).  Everything but the
// lane's own point and sums is wave-uniform.  Results go to the arena at the ray's index with plain (vector) stores.
//
// The first part of this header is plain C++17 that also compiles as HIP — the march and refinement arithmetic, the choice of the
// crossing from a sequence of sides and the argument checks (tests/host_rays/rays_main.cpp prints them on a machine without a GPU;
// sphexample_amd/rays.py restates them in numpy) — the kernel follows behind __HIPCC__.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

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

constexpr long long kMaxRays = 1ll << 20;        // SPHMI_MAX_RAYS
constexpr long long kMaxRayPoints = 1ll << 16;   // SPHMI_MAX_RAY_POINTS: march intervals per ray
constexpr int kRayRefineRounds = 4;              // SPHMI_RAY_REFINE_ROUNDS
constexpr int kRayEnter = 0, kRayLeave = 1, kRayAny = 2;      // SPHMI_RAY_ENTER, _LEAVE, _ANY
constexpr int kRayFound = 1, kRayStartsInside = 2;            // bits of status_out

// the arguments of sphmi_cast_rays behind the handle and the ray count; any output may be null
struct RayCall {
    const double *origins, *directions, *t_begin, *t_end;
    double step, level;
    int mode;
    int32_t* status;
    int64_t* interval;
    double *bracket, *point, *weight;
    int64_t* count;
    double *sum_pressure, *sum_density, *sum_velocity;
};

// x[a] = o[a] + t · d[a] for a < dims, zero beyond: one multiply, one add
SPHMI_HD void ray_point(const double* o, const double* d, double t, int dims, double* x) {
    SPHMI_NO_CONTRACT
    for (int a = 0; a < 3; ++a) {
        if (a < dims) { const double p = t * d[a]; x[a] = o[a] + p; } else x[a] = 0.0;
    }
}
// K of a ray, or −1 where it is not in [0, kMaxRayPoints] (t_end ≥ t_begin, step > 0, all finite)
inline long long ray_intervals(double t_begin, double t_end, double step) {
    const double k = ceil((t_end - t_begin) / step);
    if (!(k >= 0.0 && k <= (double)kMaxRayPoints)) return -1;
    return (long long)k;
}
// t_k, k in 0 … K
SPHMI_HD double ray_march_t(double t_begin, double t_end, double step, long long k, long long K) {
    SPHMI_NO_CONTRACT
    if (k >= K) return t_end;
    const double p = (double)k * step;
    return t_begin + p;
}
SPHMI_HD double ray_refine_delta(double a, double b) {
    SPHMI_NO_CONTRACT
    const double w = b - a;
    return w * 0.015625;
}
// u_m, m in 0 … 64
SPHMI_HD double ray_refine_u(double a, double b, double delta, int m) {
    SPHMI_NO_CONTRACT
    if (m <= 0) return a;
    if (m >= 64) return b;
    const double p = (double)m * delta;
    return a + p;
}
// do the sides of the two ends of an interval disagree the way `mode` asks?
SPHMI_HD bool ray_crosses(bool before, bool after, int mode) {
    if (before == after) return false;
    return mode == kRayAny || (mode == kRayEnter ? after : before);
}
// the crossing of a march from the sides of t_0 … t_K: the smallest k in 1 … K, or −1
inline long long ray_first_crossing(const unsigned char* inside, long long K, int mode) {
    for (long long k = 1; k <= K; ++k)
        if (ray_crosses(inside[k - 1] != 0, inside[k] != 0, mode)) return k;
    return -1;
}
// the choice of a refinement round from the sides of u_0 … u_63 (u_64 differs from u_0): the smallest m in 1 … 64
inline int ray_refine_choice(const unsigned char* inside) {
    for (int m = 1; m < 64; ++m)
        if ((inside[m] != 0) != (inside[0] != 0)) return m;
    return 64;
}

// The argument errors of sphmi_cast_rays that every kind of handle reports alike: false, and the text in `msg`, for null origins,
// directions or t_* with n_rays > 0, n_rays out of range, a non-finite coordinate or parameter (the first such ray is named), a
// zero direction, t_end < t_begin, a step or level that is not finite or ≤ 0, more than kMaxRayPoints intervals, an unknown mode.
// `K_out` (may be null) receives the intervals of every ray.
inline bool ray_check(long long n_rays, const double* origins, const double* directions, const double* t_begin, const double* t_end,
                      double step, double level, int mode, int dims, int* K_out, char* msg, size_t msg_len) {
    auto fail = [&](const char* what, long long ray) {
        if (ray >= 0) snprintf(msg, msg_len, "sphmi_cast_rays: %s at ray %lld", what, ray);
        else snprintf(msg, msg_len, "sphmi_cast_rays: %s", what);
        return false;
    };
    if (n_rays < 0 || n_rays > kMaxRays) return fail("n_rays out of range [0, SPHMI_MAX_RAYS]", -1);
    if (!(step > 0.0) || !isfinite(step)) return fail("step is not a finite number > 0", -1);
    if (!(level > 0.0) || !isfinite(level)) return fail("level is not a finite number > 0", -1);
    if (mode != kRayEnter && mode != kRayLeave && mode != kRayAny) return fail("unknown mode (SPHMI_RAY_ENTER, SPHMI_RAY_LEAVE or SPHMI_RAY_ANY)", -1);
    if (n_rays > 0 && (!origins || !directions || !t_begin || !t_end)) return fail("null origins, directions, t_begin or t_end", -1);
    for (long long r = 0; r < n_rays; ++r) {
        bool zero = true;
        for (int a = 0; a < dims; ++a) {
            if (!isfinite(origins[r * dims + a]) || !isfinite(directions[r * dims + a])) return fail("non-finite coordinate", r);
            zero = zero && directions[r * dims + a] == 0.0;
        }
        if (!isfinite(t_begin[r]) || !isfinite(t_end[r])) return fail("non-finite parameter", r);
        if (zero) return fail("zero direction", r);
        if (t_end[r] < t_begin[r]) return fail("t_end < t_begin", r);
        const long long K = ray_intervals(t_begin[r], t_end[r], step);
        if (K < 0) return fail("more than SPHMI_MAX_RAY_POINTS march intervals", r);
        if (K_out) K_out[r] = (int)K;
    }
    return true;
}

}  // namespace sphmi

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "sphmi_kernels.h"
#include "sphmi_rebuild.h"
#include "sphmi_probes.h"       // pr_kernel_w

namespace sphmi {

constexpr int kRayThreads = 256;                 // four waves: four rays per workgroup
constexpr int kRayInFlight = 2;                  // rows of a lane whose loads are issued before the first is used

template <class T> struct RayArgs {
    using V4 = typename Vec4<T>::type;
    Half<const V4> pk0, pk1;             // the set sphmi_download reads
    Half<const V4> half0;                // the half-step set: Pressure!(ρₙ⁺)
    const V4* comp;                      // fp32 handles: low words of position and density (null: none)
    const uint8_t* type;                 // slab handles: the type byte; null on plain handles
    const int* cstart;
    const double *org, *dir;             // D doubles per ray
    const double *t_begin, *t_end;
    const int* K;                        // march intervals per ray
    int* status;                         // kRayFound | kRayStartsInside
    long long* interval;                 // k, or −1
    double* bracket;                     // 2 per ray
    double* point;                       // 3 per ray
    double *S, *SP, *Sr, *Sv;            // Sv: 3 per ray
    long long* count;
    GridDesc g;
    long long n_rays;
    double H_inv, H2, h_inv, reach;
    double alphaD, m0;
    T rho0, inv_rho0, Cbe;
    int N, kernel, mode;
    double step, level;
};

// a value the compiler knows nothing about, as if it came from memory (the header comment)
__device__ __forceinline__ double ray_opaque(double v) { asm volatile("" : "+v"(v)); return v; }

// The sums of k_point_cloud at the point xp of THIS lane: s = { S, SP, Sρ, Sv[0..2], n }.  No cross-lane operation: callable
// under any exec mask.  `active` false: nothing is read, zeros.
template <class T, int D>
__device__ __forceinline__ void ray_eval(const RayArgs<T>& A, const double (&xp)[3], const bool active, double (&s)[7]) {
    using V4 = typename Vec4<T>::type;
    int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool empty = !active;
    {
#pragma clang fp contract(off)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (d >= D) continue;
            // the span of k_point_cloud for a tile of this one point
            double a = (xp[d] - A.reach) * A.H_inv, b = (xp[d] + A.reach) * A.H_inv;
            a -= 1e-6 * (1.0 + fabs(a)); b += 1e-6 * (1.0 + fabs(b));
            const double off = 1.0 - (double)A.g.gmin[d], top = (double)(A.g.np[d] - 1);
            const double l = fmax(ceil(a - 0.5) + off, 0.0), u = fmin(floor(b + 0.5) + off, top);
            if (!(l <= u) || a != a || b != b) empty = true;        // outside the grid
            lo[d] = empty ? 0 : (int)l; hi[d] = empty ? 0 : (int)u;
        }
    }
    const int ny = hi[1] - lo[1] + 1, nz = D == 3 ? hi[2] - lo[2] + 1 : 1;
    const int nrange = empty ? 0 : ny * nz;
    double n = 0.0, S = 0.0, SP = 0.0, Sr = 0.0, Sx = 0.0, Sy = 0.0, Sz = 0.0;
    int r = 0, k = 0, ke = 0;
    for (;;) {
        // the next range (cy, cz) that holds rows: its x-adjacent cells are one range of rows
        while (k >= ke && r < nrange) {
            const int cy = lo[1] + r % ny, cz = D == 3 ? lo[2] + r / ny : 0;
            const int row = A.g.np[0] * (cy + A.g.np[1] * cz);
            k = A.cstart[row + lo[0]];
            ke = A.cstart[row + hi[0] + 1];
            if (k < 0 || ke < k || ke > A.N) { k = 0; ke = 0; }     // (cannot happen on a consistent cell list; keeps every load inside the arrays)
            r += 1;
        }
        if (k >= ke) break;
        // kRayInFlight rows of the range: the cut for each, then the rest of the rows that pass, then the sums in row order
        V4 q0[kRayInFlight], lw[kRayInFlight];
        uint8_t ty[kRayInFlight];
#pragma unroll
        for (int u = 0; u < kRayInFlight; ++u) {
            const int j = min(k + u, ke - 1);
            q0[u] = A.pk0[j];
            if (sizeof(T) == 4 && A.comp) lw[u] = A.comp[j]; else { lw[u].x = lw[u].y = lw[u].z = lw[u].w = T(0); }
            ty[u] = A.type ? A.type[j] : (uint8_t)(q0[u].w > T(0) ? 1 : 2);
        }
        double r2[kRayInFlight];
        bool pass[kRayInFlight];
        V4 q1[kRayInFlight];
        T hw[kRayInFlight];
#pragma unroll
        for (int u = 0; u < kRayInFlight; ++u) {
            const bool fluid = (ty[u] & kTypeMask) == 1 && !(ty[u] & kGhostMask);      // SPHMI_FLUID, owned
            const double rx = ray_opaque((double)q0[u].x + (double)lw[u].x), ry = ray_opaque((double)q0[u].y + (double)lw[u].y),
                         rz = ray_opaque((double)q0[u].z + (double)lw[u].z);
            {
                // (no contraction: r² is ((dx² + dy²) + dz²) rounded term by term, as in k_point_cloud)
#pragma clang fp contract(off)
                const double dx = xp[0] - rx, dy = xp[1] - ry, dz = D == 3 ? xp[2] - rz : 0.0;
                r2[u] = dx * dx + dy * dy + dz * dz;
            }
            pass[u] = k + u < ke && fluid && r2[u] <= A.H2;
            const int j = pass[u] ? k + u : k;                                           // (row k is inside the arrays)
            q1[u] = A.pk1[j]; hw[u] = A.half0[j].w;
        }
#pragma unroll
        for (int u = 0; u < kRayInFlight; ++u) {
            if (pass[u]) {
                // the staging of k_point_cloud …
                const double rho = ray_opaque((double)(q0[u].w < T(0) ? -q0[u].w : q0[u].w) + (double)lw[u].w);
                const T rr = sizeof(T) == 8 ? hw[u] / A.rho0 : hw[u] * A.inv_rho0;
                const T rr2 = rr * rr, rr4 = rr2 * rr2;
                const double V = ray_opaque(A.m0 / rho);
                const double P = ray_opaque((double)(A.Cbe * (rr4 * rr2 * rr - T(1))));
                const double vx = ray_opaque((double)q1[u].x), vy = ray_opaque((double)q1[u].y), vz = ray_opaque((double)q1[u].z);
                // … and its walk
                const double w = V * pr_kernel_w(A.kernel, A.alphaD, sqrt(r2[u]) * A.h_inv);
                n += 1.0; S += w; SP += w * P; Sr += w * rho;
                Sx += w * vx; Sy += w * vy;
                if (D == 3) Sz += w * vz;
            }
        }
        k += kRayInFlight;
    }
    s[0] = S; s[1] = SP; s[2] = Sr; s[3] = Sx; s[4] = Sy; s[5] = D == 3 ? Sz : 0.0; s[6] = n;
}

template <class T, int D>
__global__ void __launch_bounds__(kRayThreads, 4) k_cast_rays(const RayArgs<T> A) {
    const int lane = (int)threadIdx.x & 63;
    const long long ray = (long long)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * (unsigned)kRayThreads + threadIdx.x) >> 6));
    if (ray >= A.n_rays) return;                                 // (the whole wave: nothing below waits for another wave)
    double o[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < D; ++a) { o[a] = A.org[ray * D + a]; d[a] = A.dir[ray * D + a]; }
    const double tb = A.t_begin[ray], te = A.t_end[ray];
    const long long K = min(max((long long)A.K[ray], 0ll), kMaxRayPoints);

    // what the wave does next — every value here is the same in all lanes
    enum { MARCH = 0, REFINE = 1, AGAIN = 2 };
    int phase = MARCH, round = 0;
    long long base = 0, crossing = -1;
    bool carry = false, side_a = false, starts_inside = false;
    double a = 0.0, b = 0.0, delta = 0.0;
    int holder = -1;                                             // the lane whose `rec` is the record of the inside end; −1: none yet
    double rec[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // the next refinement round with δ ≠ 0; false when the rounds are over
    auto next_round = [&]() {
        while (round < kRayRefineRounds) {
            delta = ray_refine_delta(a, b);
            if (delta != 0.0) return true;
            round += 1;                                          // (δ == 0: the round leaves the bracket as it is)
        }
        return false;
    };
    for (;;) {
        double t;
        bool active;
        if (phase == MARCH) { const long long k = base + lane; active = k <= K; t = ray_march_t(tb, te, A.step, k, K); }
        else if (phase == REFINE) { active = lane >= 1; t = ray_refine_u(a, b, delta, lane); }
        else { active = lane == 0; t = side_a ? a : b; }
        double x[3], s[7];
        ray_point(o, d, t, D, x);
        ray_eval<T, D>(A, x, active, s);
        const bool in = active && s[0] >= A.level;
        if (phase == MARCH) {
            const int below = __shfl_up((int)in, 1, 64);
            const bool before = lane == 0 ? carry : below != 0;
            const bool cross = active && base + lane >= 1 && ray_crosses(before, in, A.mode);
            if (base == 0) starts_inside = __shfl((int)in, 0, 64) != 0;
            const unsigned long long mask = __ballot(cross);
            if (mask == 0ull) {
                carry = __shfl((int)in, 63, 64) != 0;
                base += 64;
                if (base > K) break;                             // no crossing
                continue;
            }
            const int first = __ffsll((long long)mask) - 1;
            crossing = base + first;
            side_a = __shfl((int)before, first, 64) != 0;
            a = ray_march_t(tb, te, A.step, crossing - 1, K); b = ray_march_t(tb, te, A.step, crossing, K);
            phase = REFINE;
        } else if (phase == REFINE) {
            const unsigned long long mask = __ballot(lane >= 1 && in != side_a);
            const int m = mask == 0ull ? 64 : __ffsll((long long)mask) - 1;
            const int inside_end = side_a ? m - 1 : m;           // u_0 = a and u_64 = b are the ends the round began with
            if (inside_end >= 1 && inside_end <= 63) {
                holder = inside_end;
                if (lane == holder) {
#pragma unroll
                    for (int f = 0; f < 7; ++f) rec[f] = s[f];
                }
            }
            const double na = ray_refine_u(a, b, delta, m - 1), nb = ray_refine_u(a, b, delta, m);
            a = na; b = nb;
            round += 1;
        } else {
            if (lane == 0) {
#pragma unroll
                for (int f = 0; f < 7; ++f) rec[f] = s[f];
            }
            holder = 0;
            break;
        }
        if (!next_round()) {
            if (holder >= 0) break;
            phase = AGAIN;                                       // the inside end is the march's: lane 0 evaluates it once more
        }
    }
    const bool found = crossing >= 1;
    if (lane == (found ? holder : 0)) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        double x[3] = {nan, nan, D == 3 ? nan : 0.0};
        if (found) ray_point(o, d, side_a ? a : b, D, x);
        A.status[ray] = (found ? kRayFound : 0) | (starts_inside ? kRayStartsInside : 0);
        A.interval[ray] = found ? crossing : -1ll;
        A.bracket[2 * ray] = found ? a : nan; A.bracket[2 * ray + 1] = found ? b : nan;
        A.point[3 * ray] = x[0]; A.point[3 * ray + 1] = x[1]; A.point[3 * ray + 2] = x[2];
        A.S[ray] = found ? rec[0] : 0.0; A.SP[ray] = found ? rec[1] : 0.0; A.Sr[ray] = found ? rec[2] : 0.0;
        A.Sv[3 * ray] = found ? rec[3] : 0.0; A.Sv[3 * ray + 1] = found ? rec[4] : 0.0; A.Sv[3 * ray + 2] = found ? rec[5] : 0.0;
        A.count[ray] = found ? (long long)rec[6] : 0ll;
    }
}

}  // namespace sphmi
#endif  // __HIPCC__
