// sphmi_components.h — the connected bodies of selected rows (main body, droplets), labelled on the device on demand
// (sphmi_components_build).
//
// Two selected rows i ≠ j are linked iff r² = ((dx² + dy²) + dz²) ≤ link² — the cut of the neighbour list (sphmi_neighbor_list.h) with
// link ≤ H in the place of H, formed the same way by the same walk (nl_walk, unchanged, half = 1: every pair once).  A component is a
// connected set of selected rows; its FIRST ROW is its smallest row, and components are numbered in ascending first row.  The result
// is a function of the state alone: a host reproduces it bit for bit from a download (sphexample_amd/components.py).
//
// Five passes, all on the engine's stream:
//   k_cc_init      parent[i] = i for selected rows (bit Type of type_mask), −1 otherwise
//   k_cc_hook      the hot path: the walk of k_neighbor_count, whose accept callback unites i and j in a lock-free union–find
//   k_cc_flatten   behind the kernel boundary: root[i] = find(i) into an array of its own (no row is read while it is rewritten),
//                  flag[i] = (root[i] == i)
//   the neighbour list's scan (k_nl_tile_sums, k_nl_scan_tiles, k_nl_offsets) over the flags: C and the dense number of every root;
//   k_cc_label     label[i] = dense[root[i]], first_row[dense[i]] = i at the roots
//   k_cc_table_init, k_cc_table, k_cc_box_decode
//                  count and box of every component
//
// The union–find.  The forest keeps ONE invariant: parent[x] < x at every row that is not a root, parent[r] == r at a root.  Two
// kinds of store touch `parent`:
//   the hook    atomicCAS(&parent[hi], hi, lo) with lo < hi: it succeeds only while hi is a root, and makes it a non-root for good —
//               a row never becomes a root again.  This CAS alone decides which trees merge.
//   halving     parent[x] = g, where x was SEEN to be a non-root and g < parent[x] was seen above it: g is an ancestor of x, so the
//               store moves x inside its own tree.  It cannot collide with a hook of x (x is no root, the CAS there fails) and two
//               halving stores of one slot both leave an ancestor.
// Both keep the invariant, so the forest has no cycle, a climb descends strictly and ends after fewer than N loads, and the root of
// a tree is its smallest row.  unite(i, j) finds both roots, hooks the LARGER under the smaller, and after a failed CAS goes on from
// the value the CAS returned (the row hi hangs under now).  Every failure means another lane hooked a root; a launch holds fewer than
// N hooks, which bounds the retries.  When the kernel ends every link has been united, so trees are components and every root is
// the minimum of its component whatever the interleaving: flatten, number and table see one forest.
//   Loads on the way up are RELAXED ATOMIC loads at agent scope (they are served by the L2, like the CAS), not plain loads.  Plain
//   loads would be correct too — a stale parent out of this compute unit's L1 is a row that WAS above x, hence still in x's tree, and
//   a stale "root" fails its CAS, which returns the truth — but a stale line is re-read until it leaves the L1, so a lane could climb
//   from the same stale row again and again; the atomic loads cost the same L2 trip the CAS needs anyway and make every retry see
//   progress.  k_cc_flatten runs behind the kernel boundary and reads `parent` with plain loads: nothing writes it any more.
//   EVERY LOOP IS BOUNDED: a climb that takes more than N steps, a unite that retries more than N times or a parent outside [0, x]
//   sets a bit of the error word and ends; sphmi_components_build then returns SPHMI_ERR_DEVICE.  (Reviewed, not exercised: no
//   state reaches these bounds.)
//
// The table.  count and box come from INTEGER atomics: an int add, and 64-bit unsigned min / max on an order-preserving image of the
// position doubles (cc_key: negative doubles have all bits flipped, the others the sign bit — unsigned order is numeric order, −0
// below +0).  Integer add, min and max are associative and commutative: the result does not depend on the order of arrival, so no
// atomic decides a value.  Chosen over a counting sort by label plus a segmented pass because it needs no second scan and no permuted
// copy of the positions, and because the rows are sorted by cell: nearly every wave holds rows of ONE component, reduces them in
// registers (on the keys, so that the fast path is the same function) and issues seven atomics per wave instead of 448.
//
// LDS: k_cc_hook holds nl_walk's and nothing else (kNlLdsBytes, four workgroups per compute unit); the other kernels hold none.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_neighbor_list.h"

namespace sphmi {

constexpr int kCcThreads = 256;
enum { CC_ERR_CLIMB = 1, CC_ERR_RETRY = 2, CC_ERR_PARENT = 4 };

struct ComponentArgs {
    const uint8_t* type;
    int* parent;                         // [N]  the forest (init, hook)
    int* root;                           // [N]  the root of every selected row, −1 otherwise (flatten)
    int* flag;                           // [N]  1 at the roots (flatten); the scan reads it
    const long long* dense;              // [N + 1]  exclusive scan of the flags: the number of a root; dense[N] = C
    int* label;                          // [N]
    int* first_row;                      // [C]
    int* count;                          // [C]
    unsigned long long* box;             // [C × 6]  keys while k_cc_table runs, doubles behind k_cc_box_decode
    int* err;                            // one word, zeroed before the hook
    int N, C;
    unsigned type_mask;
};

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The root above the selected row x, with path halving.  At most N steps.
__device__ __forceinline__ int cc_find(int* parent, int x, const int N, int* err) {
    int curr = cc_load(parent + x);
    if (curr == x) return x;
    if ((unsigned)curr > (unsigned)x) { atomicOr(err, CC_ERR_PARENT); return x; }
    int prev = x;
    for (int steps = 0; ; ++steps) {
        const int next = cc_load(parent + curr);
        if (next == curr) return curr;
        if ((unsigned)next > (unsigned)curr) { atomicOr(err, CC_ERR_PARENT); return curr; }      // (never: parent[y] < y; keeps every load inside the array)
        if (steps >= N) { atomicOr(err, CC_ERR_CLIMB); return curr; }
        cc_store(parent + prev, next);                       // halving: next is an ancestor of prev, and prev is no root
        prev = curr; curr = next;
    }
}

// Unites the trees of a and b (rows of the two trees, not necessarily roots); returns a row of the united tree at or near its root.
__device__ __forceinline__ int cc_unite(int* parent, int a, int b, const int N, int* err) {
    a = cc_find(parent, a, N, err); b = cc_find(parent, b, N, err);
    for (int tries = 0; a != b; ++tries) {
        const int hi = max(a, b), lo = min(a, b);
        const int old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return lo;                            // hooked
        if (tries >= N) { atomicOr(err, CC_ERR_RETRY); return lo; }
        if ((unsigned)old > (unsigned)hi) { atomicOr(err, CC_ERR_PARENT); return lo; }
        a = cc_find(parent, old, N, err);                    // hi hangs under `old` now: go on from there
        b = cc_find(parent, lo, N, err);
    }
    return a;
}

__global__ void __launch_bounds__(kCcThreads) k_cc_init(const ComponentArgs C) {
    const int i = (int)(blockIdx.x * kCcThreads + threadIdx.x);
    if (i >= C.N) return;
    const unsigned ty = C.type[i];
    C.parent[i] = (ty < 32u && ((C.type_mask >> ty) & 1u)) ? i : -1;
}

template <class T, int D>
__global__ void __launch_bounds__(kNlThreads, 4) k_cc_hook(const NeighborListArgs<T> A, const ComponentArgs C) {
    const long long i = (long long)blockIdx.x * kNlThreads + (int)threadIdx.x;
    const bool has_row = i < (long long)A.N;
    int* const parent = C.parent;
    int* const err = C.err;
    const int N = A.N;
    int mine = has_row ? cc_load(parent + i) : -1;                    // a row of i's tree, at or near its root; −1: i takes no part
    nl_walk<T, D>(A, i, has_row, [&](int j) __attribute__((always_inline)) {
        if (mine < 0) return;
        if (cc_load(parent + j) < 0) return;                 // j is not selected
        mine = cc_unite(parent, mine, j, N, err);
    });
}

__global__ void __launch_bounds__(kCcThreads) k_cc_flatten(const ComponentArgs C) {
    const int i = (int)(blockIdx.x * kCcThreads + threadIdx.x);
    if (i >= C.N) return;
    int x = C.parent[i];
    if (x > i) { atomicOr(C.err, CC_ERR_PARENT); x = i; }    // (never: parent[i] ≤ i; keeps every load inside the array)
    if (x >= 0 && x != i) {
        for (int steps = 0; ; ++steps) {
            const int p = C.parent[x];
            if (p == x) break;
            if ((unsigned)p > (unsigned)x) { atomicOr(C.err, CC_ERR_PARENT); break; }
            if (steps >= C.N) { atomicOr(C.err, CC_ERR_CLIMB); break; }
            x = p;
        }
    }
    C.root[i] = x;
    C.flag[i] = x == i ? 1 : 0;
}

__global__ void __launch_bounds__(kCcThreads) k_cc_label(const ComponentArgs C) {
    const int i = (int)(blockIdx.x * kCcThreads + threadIdx.x);
    if (i >= C.N) return;
    const int r = C.root[i];
    int l = -1;
    if (r >= 0 && r < C.N) {
        const long long d = C.dense[r];
        if (d >= 0 && d < (long long)C.C) {
            l = (int)d;
            if (r == i) C.first_row[l] = i;
        }
    }
    C.label[i] = l;
}

// the order-preserving image of a double and its inverse
__device__ __forceinline__ unsigned long long cc_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : b ^ 0x8000000000000000ull;
}
__device__ __forceinline__ double cc_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k));
}

__global__ void __launch_bounds__(kCcThreads) k_cc_table_init(const ComponentArgs C) {
    const long long k = (long long)blockIdx.x * kCcThreads + (int)threadIdx.x;
    if (k >= 6ll * C.C) return;
    C.box[k] = (k % 6) < 3 ? ~0ull : 0ull;
    if (k < C.C) C.count[k] = 0;
}

template <class T, int D>
__global__ void __launch_bounds__(kCcThreads) k_cc_table(const NeighborListArgs<T> A, const ComponentArgs C) {
    using V4 = typename Vec4<T>::type;
    const int i = (int)(blockIdx.x * kCcThreads + threadIdx.x);
    const int l = i < C.N ? C.label[i] : -1;
    unsigned long long lo[D], hi[D];
    if (l >= 0) {
        const V4 q0 = A.pk0[i];
        V4 lw; lw.x = lw.y = lw.z = lw.w = T(0);
        if (sizeof(T) == 4 && A.comp) lw = A.comp[i];
        const double x[3] = {(double)q0.x + (double)lw.x, (double)q0.y + (double)lw.y, (double)q0.z + (double)lw.z};
#pragma unroll
        for (int d = 0; d < D; ++d) lo[d] = hi[d] = cc_key(x[d]);
    } else {
#pragma unroll
        for (int d = 0; d < D; ++d) { lo[d] = ~0ull; hi[d] = 0ull; }
    }
    const int l0 = __shfl(l, 0, 64);
    if (__all(l == l0)) {                                    // the whole wave in one component (or outside every one)
        if (l0 < 0) return;
#pragma unroll
        for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long a = (unsigned long long)__shfl_xor((long long)lo[d], o, 64), b = (unsigned long long)__shfl_xor((long long)hi[d], o, 64);
                lo[d] = a < lo[d] ? a : lo[d]; hi[d] = b > hi[d] ? b : hi[d];
            }
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(C.count + l0, 64);
#pragma unroll
            for (int d = 0; d < D; ++d) { atomicMin(C.box + 6ll * l0 + d, lo[d]); atomicMax(C.box + 6ll * l0 + 3 + d, hi[d]); }
        }
        return;
    }
    if (l < 0) return;
    atomicAdd(C.count + l, 1);
#pragma unroll
    for (int d = 0; d < D; ++d) { atomicMin(C.box + 6ll * l + d, lo[d]); atomicMax(C.box + 6ll * l + 3 + d, hi[d]); }
}

template <int D>
__global__ void __launch_bounds__(kCcThreads) k_cc_box_decode(const ComponentArgs C) {
    const long long k = (long long)blockIdx.x * kCcThreads + (int)threadIdx.x;
    if (k >= 6ll * C.C) return;
    double* const out = (double*)C.box;
    out[k] = (D == 2 && k % 3 == 2) ? 0.0 : cc_unkey(C.box[k]);
}

}  // namespace sphmi
