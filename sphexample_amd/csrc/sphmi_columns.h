// sphmi_columns.h — the caller's passive columns on the device (sphmi_attach_columns / sphmi_download_columns*).
//
// The reference's sort! permutes all 17 fields of the StructArray (src/SPHCellList.jl:142); the engine carries the ten the hot
// path touches.  The others — ChunkID, GravityFactor, MotionLimiter, BoundaryBool, GhostNormals, Kernel / KernelGradient without
// StoreKernelOutput, user columns — are opaque bytes to it: it keeps them in ONE packed record per row, in attach order, and
// never moves them.  What moves is the 4-byte row column the sorts carry anyway (Engine::prow, the row at the last
// sphmi_download_permutation) and `base`, which maps a row of that epoch to its record:
//
//     record of current row i  =  base[prow[i]]
//
//   k_columns_base_init     attach:                       base[prow[i]] = i          (the identity on a fresh epoch)
//   k_columns_base_compose  sphmi_download_permutation:   base'[i] = base[prow[i]]   (before prow becomes the identity again)
//   k_gather_columns        download:                     record → one contiguous array per column, current order
//   k_gather_selected_columns  sphmi_select_download_columns: the same for the rows of a selection, record of base[prow[rows[s]]]
//
// Record layout: the columns of a row side by side, the wider-aligned first (a width divisible by 16, then by 8, 4, 2, then
// the odd ones), so every column whose width is a multiple of 4 starts on a 4-byte boundary without padding; the stride is
// the sum of the widths rounded up to 16 bytes.  Late in a run the record order is random with respect to the row order: a
// gather then touches one or two 128-byte lines per row instead of one per column.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sphmi_series.h"      // kMaxColumns, kMaxColumnRowBytes

namespace sphmi {

constexpr int kGatherThreads = 256;
constexpr int kGatherLdsBytes = 32768;   // records + source rows of one block

// by value in the kernel arguments
struct ColumnTable {
    int n_columns;
    int stride;                          // bytes per record, a multiple of 16
    int rows_per_block;                  // a multiple of 16: the bytes a block writes per column start 16-byte aligned
    int reserved;
    int offset[kMaxColumns];             // of column c inside the record
    int width[kMaxColumns];              // row_bytes of column c
    char* out[kMaxColumns];              // n × width[c] bytes, 16-byte aligned; nullptr: the caller skips this column
};

inline int gather_rows_per_block(int stride) {
    const int r = (kGatherLdsBytes / (stride + 4)) / 16 * 16;
    return r < 16 ? 16 : (r > kGatherThreads ? kGatherThreads : r);
}
inline size_t gather_lds_bytes(const ColumnTable& t) { return (size_t)t.rows_per_block * (size_t)(t.stride + 4); }

// prow is a permutation of 0 … n − 1 (one-device handles; slab engines never attach columns); the range tests keep a
// corrupted column from turning into a wild store
__global__ void k_columns_base_init(const int* __restrict__ prow, int* __restrict__ base, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned e = (unsigned)prow[i];
    if (e < (unsigned)n) base[e] = i;
}

__global__ void k_columns_base_compose(const int* __restrict__ base_in, const int* __restrict__ prow, int* __restrict__ base_out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned e = (unsigned)prow[i];
    base_out[i] = e < (unsigned)n ? base_in[e] : -1;
}

// One block delivers rows_per_block consecutive rows.  (1) the record index of every row → LDS; (2) the records → LDS with
// 16-byte loads, stride / 16 consecutive lanes per record, so a wave's load instruction covers whole records; (3) per column
// the block's rows are ONE contiguous byte range of the output: it is written in dwords by consecutive lanes — a column whose
// width and offset are multiples of 4 reads one LDS dword per store, any other (1-, 2-, 3-, 7-, 33-byte rows) assembles a
// dword from four LDS bytes, which may belong to four rows: a 1-byte column costs a quarter store per row, not one.
// `kRows`: the block delivers the rows sel[row0 …] of a selection (k_gather_selected_columns) instead of the rows row0 … themselves;
// `n` is then the number of selected rows and `n_src` the number of rows of the handle.
template <bool kRows>
__device__ __forceinline__ void gather_columns_block(const uint4* __restrict__ store, const int* __restrict__ base, const int* __restrict__ prow,
                                                     const int* __restrict__ sel, int n, int n_src, const ColumnTable& t) {
    extern __shared__ uint4 gather_lds[];
    const int R = t.rows_per_block, S = t.stride, L = S >> 4;
    int* src = (int*)gather_lds;                       // R ints (R is a multiple of 16: the records behind them stay 16-byte aligned)
    uint4* recs = gather_lds + (R >> 2);               // R records
    const int tid = (int)threadIdx.x;
    const int row0 = (int)blockIdx.x * R;
    const int rows = min(R, n - row0);
    for (int r = tid; r < rows; r += kGatherThreads) {
        unsigned i = (unsigned)(row0 + r);
        if (kRows) i = (unsigned)sel[row0 + r];
        const unsigned e = i < (unsigned)n_src ? (unsigned)prow[i] : ~0u;
        const int s = e < (unsigned)n_src ? base[e] : -1;
        src[r] = (unsigned)s < (unsigned)n_src ? s : -1;
    }
    __syncthreads();
    for (int g = tid; g < rows * L; g += kGatherThreads) {
        const int r = g / L, q = g - r * L;
        const int s = src[r];
        recs[g] = s >= 0 ? store[(size_t)s * (size_t)L + (size_t)q] : uint4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    const unsigned char* rb = (const unsigned char*)recs;
    const unsigned* rw = (const unsigned*)recs;
    for (int c = 0; c < t.n_columns; ++c) {
        char* out = t.out[c];
        if (!out) continue;
        const int w = t.width[c], off = t.offset[c];
        out += (size_t)row0 * (size_t)w;
        const int bytes = rows * w, nd = bytes >> 2;
        if (((w | off) & 3) == 0) {
            const int m = w >> 2, o4 = off >> 2, s4 = S >> 2;
            for (int d = tid; d < nd; d += kGatherThreads) {
                const int r = d / m;
                ((unsigned*)out)[d] = rw[r * s4 + o4 + (d - r * m)];
            }
        } else {
            for (int d = tid; d < nd; d += kGatherThreads) {
                unsigned v = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int o = 4 * d + k, r = o / w;
                    v |= (unsigned)rb[r * S + off + (o - r * w)] << (8 * k);
                }
                ((unsigned*)out)[d] = v;
            }
            for (int o = (nd << 2) + tid; o < bytes; o += kGatherThreads) {        // (the last block of a column whose byte count is no multiple of 4)
                const int r = o / w;
                out[o] = (char)rb[r * S + off + (o - r * w)];
            }
        }
    }
}

__global__ void __launch_bounds__(kGatherThreads)
k_gather_columns(const uint4* __restrict__ store, const int* __restrict__ base, const int* __restrict__ prow, int n, ColumnTable t) {
    gather_columns_block<false>(store, base, prow, nullptr, n, n, t);
}

// the columns of the selected rows sel[0 … n_sel) (sphmi_select.h), n_sel × width[c] bytes per column
__global__ void __launch_bounds__(kGatherThreads)
k_gather_selected_columns(const uint4* __restrict__ store, const int* __restrict__ base, const int* __restrict__ prow, const int* __restrict__ sel,
                          int n_sel, int n, ColumnTable t) {
    gather_columns_block<true>(store, base, prow, sel, n_sel, n, t);
}

}  // namespace sphmi
