// sphmi_group_forces.h — the per-step force on particle groups, recorded on the device (sphmi_group_forces_enable / _read).
//
// For every EXECUTED step and every selected GroupMarker g:   F_g = m₀ · Σ_{rows i the handle owns, GroupMarker[i] = g} Acceleration[i]
// with Acceleration what sphmi_download would deliver directly after that step (the corrector's value, gravity included), summed
// in fp64 on fp32 and fp64 handles alike.  An impact peak lasts a few steps and an output interval hundreds; a download per step
// costs several steps — so the series is produced inside the queued steps and travels with the control block of a batch.
//
//   at every rebuild that permutes (and at enable): the rows of the selected groups, one compact list, row order kept
//     k_gf_count     rows of group g in every block of 256 rows
//     k_gf_offsets   one workgroup: exclusive scan per group; group g's list starts on a multiple of kGfChunk entries
//     k_gf_fill      the rows, at their block's offset + their rank in the block
//   behind every corrector (Engine::gf_sample):
//     k_gf_partial   chunk c = kGfChunk list entries of ONE group → partial[c] = Σ a, a fixed tree: lanes (butterfly), then waves 0 … 3
//     k_gf_final     one wave: the partials of a group, lane l taking chunks l, l + 64, … in order, then the butterfly; one record
//     k_gf_small     both stages in one launch of one workgroup (handles of at most kGfSmallRows rows: a launch costs more than the sum)
//
// The order of every sum is a function of the row lists alone — no atomics on floating-point values, nothing depends on the grid
// of the launch, on the tile schedule or on timing — and k_gf_small adds in exactly the order of the two-stage pair.
// All three return at once when the step was cancelled (StepCtrl::active == 0), like the pass kernels.
//
// Record (StepRecord, sphmi_step_record.h; kStepHeader + 3·n_groups doubles): the header, then F[g][0..2]; 2-D handles write a zero
// third component.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_kernels.h"
#include "sphmi_rebuild.h"
#include "sphmi_series.h"       // kMaxForceGroups
#include "sphmi_step_record.h"  // StepRecord, wave_sum

namespace sphmi {

constexpr int kGfChunk = 256;            // list entries per partial sum = threads of the workgroup that forms it
constexpr int kGfRecordMax = kStepHeader + 3 * kMaxForceGroups;
constexpr int kGfSmallChunks = 96;       // k_gf_small keeps the partials in LDS: rows / kGfChunk + n_groups chunks at most
constexpr int kGfSmallRows = (kGfSmallChunks - kMaxForceGroups) * kGfChunk;

// by value in the kernel arguments
struct GroupTable {
    int n, reserved;
    unsigned long long marker[kMaxForceGroups];
};
// device-side description of the list: chunk0[g] … chunk0[g + 1] − 1 are the chunks of group g (chunk0[n] = all chunks), rows[g] its rows
struct GroupListMeta {
    int chunk0[kMaxForceGroups + 1];
    int rows[kMaxForceGroups];
};

__device__ __forceinline__ int gf_group_of(const GroupTable& t, unsigned long long marker, uint8_t type) {
    if (type == 0 || (type & kGhostMask)) return -1;        // dead rows and ghost copies of a slab handle are not the handle's own
    int g = -1;
    for (int k = 0; k < t.n; ++k) g = marker == t.marker[k] ? k : g;
    return g;
}

// counts[g · nblk + b] = rows of group g among rows 256·b … 256·b + 255
__global__ void __launch_bounds__(256) k_gf_count(const unsigned long long* __restrict__ grp, const uint8_t* __restrict__ type, int N,
                                                  GroupTable t, int nblk, int* __restrict__ counts) {
    __shared__ int s_cnt[4][kMaxForceGroups];
    const int i = blockIdx.x * 256 + (int)threadIdx.x, wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int g = i < N ? gf_group_of(t, grp[i], type[i]) : -1;
    for (int k = 0; k < t.n; ++k) {
        const unsigned long long b = __ballot(g == k);
        if (lane == 0) s_cnt[wave][k] = __popcll(b);
    }
    __syncthreads();
    if ((int)threadIdx.x < t.n) {
        const int k = (int)threadIdx.x;
        counts[(size_t)k * nblk + blockIdx.x] = s_cnt[0][k] + s_cnt[1][k] + s_cnt[2][k] + s_cnt[3][k];
    }
}

// one workgroup of 1024: offsets[g · nblk + b] = first list entry of block b's rows of group g
__global__ void __launch_bounds__(1024) k_gf_offsets(const int* __restrict__ counts, int nblk, int n_groups, int* __restrict__ offsets,
                                                     GroupListMeta* __restrict__ meta) {
    __shared__ int s_scan[1024];
    __shared__ int s_carry;
    const int tid = (int)threadIdx.x;
    int chunk = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (tid == 0) s_carry = 0;
        __syncthreads();
        for (int b0 = 0; b0 < nblk; b0 += 1024) {
            const int b = b0 + tid;
            const int v = b < nblk ? counts[(size_t)g * nblk + b] : 0;
            s_scan[tid] = v;
            __syncthreads();
            for (int d = 1; d < 1024; d <<= 1) {
                const int u = tid >= d ? s_scan[tid - d] : 0;
                __syncthreads();
                s_scan[tid] += u;
                __syncthreads();
            }
            const int carry = s_carry;
            if (b < nblk) offsets[(size_t)g * nblk + b] = chunk * kGfChunk + carry + s_scan[tid] - v;
            __syncthreads();
            if (tid == 1023) s_carry = carry + s_scan[1023];
            __syncthreads();
        }
        const int rows = s_carry;
        if (tid == 0) { meta->chunk0[g] = chunk; meta->rows[g] = rows; }
        chunk += (rows + kGfChunk - 1) / kGfChunk;
        __syncthreads();
    }
    if (tid == 0) meta->chunk0[n_groups] = chunk;
}

// list_cap: entries of `list` (N + n_groups · kGfChunk); a count that does not fit the list cannot come out of k_gf_count — the test keeps
// a corrupted table from turning into a wild store
__global__ void __launch_bounds__(256) k_gf_fill(const unsigned long long* __restrict__ grp, const uint8_t* __restrict__ type, int N,
                                                 GroupTable t, int nblk, const int* __restrict__ offsets, int* __restrict__ list, int list_cap) {
    __shared__ int s_cnt[4][kMaxForceGroups];
    const int i = blockIdx.x * 256 + (int)threadIdx.x, wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int g = i < N ? gf_group_of(t, grp[i], type[i]) : -1;
    int rank = 0;
    for (int k = 0; k < t.n; ++k) {
        const unsigned long long b = __ballot(g == k);
        if (lane == 0) s_cnt[wave][k] = __popcll(b);
        if (g == k) rank = __popcll(b & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    if (g < 0) return;
    for (int w = 0; w < wave; ++w) rank += s_cnt[w][g];
    const int at = offsets[(size_t)g * nblk + blockIdx.x] + rank;
    if ((unsigned)at < (unsigned)list_cap) list[at] = i;
}

// the workgroup's 256 threads form the sum of chunk c; thread 0 returns it (s_w: 4 × 3 doubles of LDS, free again on return)
template <class T>
__device__ __forceinline__ void gf_chunk_sum(const typename Vec4<T>::type* __restrict__ acc, const int* __restrict__ list,
                                             const GroupListMeta* __restrict__ meta, int n_groups, int N, int c, double (*s_w)[3], double out[3]) {
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int g = 0;
    for (int k = 1; k < n_groups; ++k) g = c >= meta->chunk0[k] ? k : g;
    const int k = (c - meta->chunk0[g]) * kGfChunk + tid;
    double x = 0.0, y = 0.0, z = 0.0;
    if (k < meta->rows[g]) {
        const unsigned row = (unsigned)list[(size_t)c * kGfChunk + tid];
        if (row < (unsigned)N) { const auto a = acc[row]; x = (double)a.x; y = (double)a.y; z = (double)a.z; }
    }
    x = wave_sum(x); y = wave_sum(y); z = wave_sum(z);
    if (lane == 0) { s_w[wave][0] = x; s_w[wave][1] = y; s_w[wave][2] = z; }
    __syncthreads();
    if (tid == 0)
        for (int d = 0; d < 3; ++d) out[d] = ((s_w[0][d] + s_w[1][d]) + s_w[2][d]) + s_w[3][d];
    __syncthreads();
}

struct GroupSampleArgs {
    StepRecord step;
    const int* list;
    const GroupListMeta* meta;
    double* partial;                 // 3 doubles per chunk
    double m0;
    int n_groups, N, D;
};

// one wave: the record of this step from the partials (global memory or LDS)
__device__ __forceinline__ void gf_write_record(const GroupSampleArgs& A, const StepCtrl& c, const double* partial, const GroupListMeta* meta) {
    const int lane = (int)threadIdx.x & 63;
    const long long slot = A.step.slot(c);
    if (slot < 0) return;
    double* rec = A.step.at(slot);
    if (lane == 0) A.step.write_header(rec, c);
    for (int g = 0; g < A.n_groups; ++g) {
        double x = 0.0, y = 0.0, z = 0.0;
        for (int ch = meta->chunk0[g] + lane; ch < meta->chunk0[g + 1]; ch += 64) { x += partial[3 * ch]; y += partial[3 * ch + 1]; z += partial[3 * ch + 2]; }
        x = wave_sum(x); y = wave_sum(y); z = wave_sum(z);
        if (lane == 0) {
            rec[kStepHeader + 3 * g] = A.m0 * x;
            rec[kStepHeader + 3 * g + 1] = A.m0 * y;
            rec[kStepHeader + 3 * g + 2] = A.D == 3 ? A.m0 * z : 0.0;
        }
    }
}

// any grid: workgroup b takes chunks b, b + gridDim.x, …
template <class T>
__global__ void __launch_bounds__(kGfChunk) k_gf_partial(const typename Vec4<T>::type* __restrict__ acc, GroupSampleArgs A, int max_chunks) {
    if (!A.step.ctrl->active) return;
    __shared__ double s_w[4][3];
    const int nchunk = min(A.meta->chunk0[A.n_groups], max_chunks);
    for (int c = (int)blockIdx.x; c < nchunk; c += (int)gridDim.x) {
        double s[3];
        gf_chunk_sum<T>(acc, A.list, A.meta, A.n_groups, A.N, c, s_w, s);
        if (threadIdx.x == 0) { A.partial[3 * c] = s[0]; A.partial[3 * c + 1] = s[1]; A.partial[3 * c + 2] = s[2]; }
    }
}
__global__ void __launch_bounds__(64) k_gf_final(GroupSampleArgs A) {
    const StepCtrl c = *A.step.ctrl;
    if (!c.active) return;
    gf_write_record(A, c, A.partial, A.meta);
}
// one workgroup: the chunks one after the other, the partials in LDS, wave 0 writes the record
template <class T>
__global__ void __launch_bounds__(kGfChunk) k_gf_small(const typename Vec4<T>::type* __restrict__ acc, GroupSampleArgs A) {
    const StepCtrl c = *A.step.ctrl;
    if (!c.active) return;
    __shared__ double s_w[4][3];
    __shared__ double s_partial[3 * kGfSmallChunks];
    const int nchunk = min(A.meta->chunk0[A.n_groups], kGfSmallChunks);
    for (int ch = 0; ch < nchunk; ++ch) {
        double s[3];
        gf_chunk_sum<T>(acc, A.list, A.meta, A.n_groups, A.N, ch, s_w, s);
        if (threadIdx.x == 0) { s_partial[3 * ch] = s[0]; s_partial[3 * ch + 1] = s[1]; s_partial[3 * ch + 2] = s[2]; }
    }
    __syncthreads();
    if (threadIdx.x < 64) gf_write_record(A, c, s_partial, A.meta);
}

}  // namespace sphmi
