// sphmi_iso_core.h — the free surface as a mesh: what ONE node and ONE cell of the lattice do (sphmi_isosurface_build).  Plain C++17
// that also compiles as HIP: the kernels of sphmi_isosurface.h call these functions one lane per node, and
// tests/host_isosurface/iso_main.cpp calls them in a loop on a machine without a GPU.  No HIP header, no other header of the engine.
//
// The field is the Shepard sum S of sphmi_sample_grid, node (i, j, k) at origin[d] + (double)i_d · spacing[d], index
// i + nx · (j + ny · k).  Node n is INSIDE iff S[n] >= level.
//
// Kuhn simplices.  Every cell — named by its lowest node — is cut into D! simplices along its main diagonal: for an axis permutation π,
// w₀ = the lowest corner, w_k = w_{k−1} + e_{π(k)}; two triangles in 2-D, six tetrahedra in 3-D, in the lexicographic order of π.  A
// corner of the cell is named by its bitmask of unit steps (bit d: one step along axis d), so the corners of a simplex are a chain of
// masks 0 ⊂ … ⊂ 2^D − 1, and neighbouring cells agree on every face diagonal: the surface is watertight without special cases.
//
// Edges.  An edge joins node a to b = a + m, m ∈ 1 … 2^D − 1 a bitmask of unit steps; a OWNS it, in slot m − 1; it exists if b is on the
// lattice and crosses iff exactly one end is inside.  Every edge of a simplex is such an edge, owned by its corner of lower position,
// and every edge of a lattice with cells lies in a simplex.  (A lattice with a count of 1 along an axis has no cells: it has no edges
// either, and its mesh is empty.)
// One vertex per crossing edge, at x_a + t · (x_b − x_a), t = (level − S_a) / (S_b − S_a), always from the owner, every operation
// rounded once (no contraction).  Vertex order: owner ascending, then slot ascending — the index of an edge's vertex is
// voff[owner] + popcount(mask[owner] & ((1 << slot) − 1)): no hash table, no atomics.
//
// Elements, per simplex by its inside set (positions 0 … D in w):
//   3-D, one corner inside or one outside: that corner a; the triangle of the edges (a, b), b ≠ a ascending.
//   3-D, two inside a < b, two outside c < d: [(a,c), (a,d), (b,d)] then [(a,c), (b,d), (b,c)].
//     The first vertex stays; the other two are swapped where needed so that (v₁ − v₀) × (v₂ − v₀) points from the inside corners to
//     the outside ones, out of the fluid.
//   2-D: the segment between the two crossing edges, directed so that the inside lies to its left.
// The swap depends on (π, inside set) alone — inside a simplex the surface is the level set of a linear function, whose gradient
// points from the outside corners to the inside ones wherever the vertices lie on their edges — so it is decided ONCE, with every
// vertex at the middle of its edge in integer arithmetic, when the table below is made (make_iso_table, constexpr).  Degenerate
// elements (t = 0: a node exactly at the level) are legal and kept.
//
// Attributes at a vertex: A_a + t · (A_b − A_a) of the lattice means SP / S and Sv / S (one IEEE division each, 0 where n == 0 or
// S <= 0 — kernel_mean of sphmi_series.h); if exactly one end has n == 0 the other end's mean is taken unmixed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SPHMI_HD __host__ __device__ inline
#else
#define SPHMI_HD inline
#endif
#if defined(__clang__)
#define SPHMI_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SPHMI_NO_CONTRACT                        /* (the host program is compiled with -ffp-contract=off) */
#endif

namespace sphmi {

// ---- the table: (simplex, inside set) → elements ------------------------------------------------------------------------------------
template <int D> struct IsoTable {
    static constexpr int kSimplices = D == 3 ? 6 : 2, kCorners = D + 1, kSets = 1 << (D + 1), kMaxElements = D == 3 ? 2 : 1;
    unsigned char perm[kSimplices][D];                               // π, lexicographic
    unsigned char corner[kSimplices][kCorners];                      // the corner masks of w₀ … w_D
    unsigned char count[kSimplices][kSets];                          // elements by inside set (bit k: w_k is inside)
    unsigned char vertex[kSimplices][kSets][kMaxElements][D];        // per element vertex, its edge: (owner's corner mask << 3) | slot
    unsigned char swapped[kSimplices][kSets];                        // bit e: element e's last two vertices were swapped
    bool undecided;                                                  // a swap the middle-of-edge geometry could not decide (never)
};

template <int D> constexpr IsoTable<D> make_iso_table() {
    IsoTable<D> T{};
    // π in lexicographic order: the D-digit numbers in base D whose digits are distinct, ascending
    int ns = 0, total = 1;
    for (int d = 0; d < D; ++d) total *= D;
    for (int code = 0; code < total; ++code) {
        int p[3] = {0, 0, 0}, c = code;
        for (int k = D - 1; k >= 0; --k) { p[k] = c % D; c /= D; }
        bool distinct = true;
        for (int a = 0; a < D; ++a) for (int b = 0; b < a; ++b) if (p[a] == p[b]) distinct = false;
        if (!distinct) continue;
        T.corner[ns][0] = 0;
        for (int k = 0; k < D; ++k) { T.perm[ns][k] = (unsigned char)p[k]; T.corner[ns][k + 1] = (unsigned char)(T.corner[ns][k] | (1 << p[k])); }
        ns += 1;
    }
    for (int s = 0; s < T.kSimplices; ++s) {
        for (int set = 1; set < T.kSets - 1; ++set) {
            int in[4] = {}, out[4] = {}, ni = 0, no = 0;
            for (int k = 0; k <= D; ++k) { if ((set >> k) & 1) in[ni++] = k; else out[no++] = k; }
            // the elements as pairs of positions, before the swap
            int e[2][3][2] = {}, ne = 0;
            if (D == 3) {
                if (ni == 1 || no == 1) {
                    const int a = ni == 1 ? in[0] : out[0];
                    int v = 0;
                    for (int b = 0; b <= D; ++b) if (b != a) { e[0][v][0] = a; e[0][v][1] = b; v += 1; }
                    ne = 1;
                } else {
                    const int a = in[0], b = in[1], c = out[0], d = out[1];
                    const int q[2][3][2] = {{{a, c}, {a, d}, {b, d}}, {{a, c}, {b, d}, {b, c}}};
                    for (int t = 0; t < 2; ++t) for (int v = 0; v < 3; ++v) { e[t][v][0] = q[t][v][0]; e[t][v][1] = q[t][v][1]; }
                    ne = 2;
                }
            } else {
                int v = 0;
                for (int a = 0; a <= D; ++a) for (int b = a + 1; b <= D; ++b) if (((set >> a) & 1) != ((set >> b) & 1)) { e[0][v][0] = a; e[0][v][1] = b; v += 1; }
                ne = 1;
            }
            // the direction from the inside corners to the outside ones: ni · Σ out − no · Σ in, in units of the cell
            int dir[3] = {0, 0, 0};
            for (int d = 0; d < D; ++d) {
                for (int k = 0; k < no; ++k) dir[d] += ni * ((T.corner[s][out[k]] >> d) & 1);
                for (int k = 0; k < ni; ++k) dir[d] -= no * ((T.corner[s][in[k]] >> d) & 1);
            }
            T.count[s][set] = (unsigned char)ne;
            for (int t = 0; t < ne; ++t) {
                int x[3][3] = {};                                    // twice the middle of every edge: the sum of its two corners
                for (int v = 0; v < D; ++v) for (int d = 0; d < D; ++d) x[v][d] = ((T.corner[s][e[t][v][0]] >> d) & 1) + ((T.corner[s][e[t][v][1]] >> d) & 1);
                int side = 0;
                if (D == 3) {
                    int u[3] = {}, w[3] = {};
                    for (int d = 0; d < 3; ++d) { u[d] = x[1][d] - x[0][d]; w[d] = x[2][d] - x[0][d]; }
                    const int n[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
                    side = n[0] * dir[0] + n[1] * dir[1] + n[2] * dir[2];                 // > 0: the normal points out of the fluid
                } else {
                    const int u[2] = {x[1][0] - x[0][0], x[1][1] - x[0][1]};
                    side = -(u[0] * dir[1] - u[1] * dir[0]);                             // > 0: the outside lies to the right, the inside to the left
                }
                if (side == 0) T.undecided = true;
                const bool swap = side < 0;
                if (swap) {
                    T.swapped[s][set] |= (unsigned char)(1 << t);
                    for (int k = 0; k < 2; ++k) { const int h = e[t][D - 2][k]; e[t][D - 2][k] = e[t][D - 1][k]; e[t][D - 1][k] = h; }
                }
                for (int v = 0; v < D; ++v) {
                    const int lo = e[t][v][0] < e[t][v][1] ? e[t][v][0] : e[t][v][1], hi = e[t][v][0] < e[t][v][1] ? e[t][v][1] : e[t][v][0];
                    const int owner = T.corner[s][lo], m = T.corner[s][hi] ^ T.corner[s][lo];
                    T.vertex[s][set][t][v] = (unsigned char)((owner << 3) | (m - 1));
                }
            }
        }
    }
    return T;
}
static_assert(!make_iso_table<2>().undecided && !make_iso_table<3>().undecided, "every swap is decided by the middle-of-edge geometry");

template <int D> SPHMI_HD const IsoTable<D>& iso_table() {
    static constexpr IsoTable<D> T = make_iso_table<D>();
    return T;
}

// the inside set of simplex s (bit k: w_k inside) out of the cell's corner set (bit c: the corner of mask c inside)
template <int D> SPHMI_HD int iso_inside_set(const IsoTable<D>& T, int s, unsigned corners) {
    int set = 0;
    for (int k = 0; k <= D; ++k) set |= (int)((corners >> T.corner[s][k]) & 1u) << k;
    return set;
}
template <int D> SPHMI_HD int iso_cell_count(unsigned corners) {
    const IsoTable<D>& T = iso_table<D>();
    int n = 0;
    for (int s = 0; s < T.kSimplices; ++s) n += T.count[s][iso_inside_set<D>(T, s, corners)];
    return n;
}
SPHMI_HD int iso_popcount(unsigned v) { int n = 0; for (; v; v &= v - 1) n += 1; return n; }

// ---- the arithmetic: every operation rounded once ------------------------------------------------------------------------------------
SPHMI_HD double iso_coord(double origin, int i, double spacing) { SPHMI_NO_CONTRACT const double step = (double)i * spacing; return origin + step; }
SPHMI_HD double iso_t(double level, double Sa, double Sb) { SPHMI_NO_CONTRACT const double num = level - Sa, den = Sb - Sa; return num / den; }
SPHMI_HD double iso_lerp(double a, double b, double t) { SPHMI_NO_CONTRACT const double d = b - a; const double td = t * d; return a + td; }
SPHMI_HD double iso_mean(double sum, double S, bool some) { return some ? sum / S : 0.0; }      // kernel_mean of sphmi_series.h

// ---- the passes, per node --------------------------------------------------------------------------------------------------------------
// What every pass sees.  `sums`: the arena k_field_grid leaves, field f of node n at sums[f · nodes + n], f = 0 S, 1 SP, 3 … 5 Sv, 6 n.
struct IsoArgs {
    const double* sums;
    double origin[3], spacing[3], level;
    int counts[3];                              // (1 along the axes a 2-D handle does not have)
    int nodes;                                  // at most SPHMI_MAX_GRID_NODES = 2²⁴
    unsigned char *mask, *corners;              // [nodes]  the crossing edges a node owns; the inside set of the corners of the cell it names
    int *vcount, *ecount;                       // [nodes]  vertices a node owns, elements of the cell it names
    const long long *voff, *eoff;               // [nodes + 1]  their exclusive scans
    double *vertices, *pressure, *velocity;     // [nv × 3], [nv], [nv × 3]  (either attribute array may be null: not formed)
    int* elements;                              // [ne × D]
};

struct IsoNode { int idx[3]; bool step[3]; };   // where a node is, and along which axes it has a neighbour above
template <int D> SPHMI_HD IsoNode iso_node(const IsoArgs& A, int node) {
    IsoNode n{};
    int r = node;
    for (int d = 0; d < 3; ++d) {
        n.idx[d] = d < D ? r % A.counts[d] : 0;
        if (d < D) r /= A.counts[d];
        n.step[d] = d < D && n.idx[d] + 1 < A.counts[d];
    }
    return n;
}
template <int D> SPHMI_HD int iso_offset(const IsoArgs& A, int m) {      // the index distance of the node m steps away
    int off = 0, stride = 1;
    for (int d = 0; d < D; ++d) { if ((m >> d) & 1) off += stride; stride *= A.counts[d]; }
    return off;
}
template <int D> SPHMI_HD bool iso_exists(const IsoArgs& A, const IsoNode& n, int m) {
    bool on = true;
    for (int d = 0; d < D; ++d) if ((((m >> d) & 1) && !n.step[d]) || A.counts[d] < 2) on = false;      // (a count of 1: no cells, no edges, an empty mesh)
    return on;
}

// pass 1: the edge mask of the node, its vertex count, and — a node that names a cell — the cell's corner set and element count
template <int D> SPHMI_HD void iso_classify_node(const IsoArgs& A, int node) {
    const IsoNode n = iso_node<D>(A, node);
    const bool in_a = A.sums[node] >= A.level;
    unsigned mask = 0, corners = in_a ? 1u : 0u;
    bool cell = true;
    for (int m = 1; m < (1 << D); ++m) {
        if (!iso_exists<D>(A, n, m)) { cell = false; continue; }
        const bool in_b = A.sums[node + iso_offset<D>(A, m)] >= A.level;
        if (in_b) corners |= 1u << m;
        if (in_b != in_a) mask |= 1u << (m - 1);
    }
    A.mask[node] = (unsigned char)mask;
    A.vcount[node] = iso_popcount(mask);
    A.corners[node] = (unsigned char)(cell ? corners : 0u);          // (no corner inside: no element)
    A.ecount[node] = cell ? iso_cell_count<D>(corners) : 0;
}

// pass 3: the vertices of the node's crossing edges, slot ascending, at voff[node] + rank
template <int D> SPHMI_HD void iso_node_vertices(const IsoArgs& A, int node) {
    const unsigned mask = A.mask[node];
    if (!mask) return;
    const IsoNode n = iso_node<D>(A, node);
    const size_t N = (size_t)A.nodes;
    const double Sa = A.sums[node], na = A.sums[6 * N + node];
    const bool some_a = na > 0.0 && Sa > 0.0;
    double xa[3], Aa[4] = {0.0, 0.0, 0.0, 0.0};
    for (int d = 0; d < 3; ++d) xa[d] = d < D ? iso_coord(A.origin[d], n.idx[d], A.spacing[d]) : 0.0;
    const bool attributes = A.pressure || A.velocity;
    if (attributes) {
        Aa[0] = iso_mean(A.sums[1 * N + node], Sa, some_a);
        for (int d = 0; d < 3; ++d) Aa[1 + d] = iso_mean(A.sums[(3 + d) * N + node], Sa, some_a);
    }
    long long at = A.voff[node];
    const long long end = A.voff[node + 1];
    for (int m = 1; m < (1 << D); ++m) {
        if (!((mask >> (m - 1)) & 1u)) continue;
        if (at >= end) return;                                      // (cannot happen: the count is the popcount of this mask)
        const int b = node + iso_offset<D>(A, m);
        const double Sb = A.sums[b];
        const double t = iso_t(A.level, Sa, Sb);
        for (int d = 0; d < 3; ++d) {
            const double xb = d < D ? iso_coord(A.origin[d], n.idx[d] + ((m >> d) & 1), A.spacing[d]) : 0.0;
            A.vertices[3 * at + d] = d < D ? iso_lerp(xa[d], xb, t) : 0.0;
        }
        if (attributes) {
            const double nb = A.sums[6 * N + b];
            const bool some_b = nb > 0.0 && Sb > 0.0, none_a = !(na > 0.0), none_b = !(nb > 0.0);
            const double Pb = iso_mean(A.sums[1 * N + b], Sb, some_b);
            if (A.pressure) A.pressure[at] = none_a != none_b ? (none_a ? Pb : Aa[0]) : iso_lerp(Aa[0], Pb, t);
            if (A.velocity)
                for (int d = 0; d < 3; ++d) {
                    const double Vb = iso_mean(A.sums[(3 + d) * N + b], Sb, some_b);
                    A.velocity[3 * at + d] = none_a != none_b ? (none_a ? Vb : Aa[1 + d]) : iso_lerp(Aa[1 + d], Vb, t);
                }
        }
        at += 1;
    }
}

// pass 4: the elements of the cell the node names, at eoff[node]: simplices in the order of π, vertex indices by owner and slot
template <int D> SPHMI_HD void iso_cell_elements(const IsoArgs& A, int node) {
    long long at = A.eoff[node];
    const long long end = A.eoff[node + 1];
    if (at >= end) return;
    const IsoTable<D>& T = iso_table<D>();
    const unsigned corners = A.corners[node];
    for (int s = 0; s < T.kSimplices; ++s) {
        const int set = iso_inside_set<D>(T, s, corners);
        for (int e = 0; e < T.count[s][set]; ++e) {
            if (at >= end) return;                                  // (cannot happen: the count pass read the same table)
            for (int v = 0; v < D; ++v) {
                const int code = T.vertex[s][set][e][v], slot = code & 7;
                const int owner = node + iso_offset<D>(A, code >> 3);
                A.elements[D * at + v] = (int)(A.voff[owner] + iso_popcount(A.mask[owner] & ((1u << slot) - 1u)));
            }
            at += 1;
        }
    }
}

}  // namespace sphmi
