// The free-surface extraction (sphexample_amd/csrc/sphmi_iso_core.h) run on the host: the passes of sphmi_isosurface_build — classify,
// two exclusive scans, vertices, elements — as plain loops over the nodes of a lattice read from a file, calling the very functions
// the kernels of sphmi_isosurface.h call one lane per node.  Built with the host compiler (and the address / undefined-behaviour
// sanitizers where their runtime links) by tests/test_isosurface_host.py, run as a child process.
//
//   iso_main --table                 prints, per dimension, one line per (simplex, inside set): "D s π set count swapped v…"
//   iso_main IN OUT                  IN:  int64 dims, int64 counts[3], double origin[3], spacing[3], level, then the 7 raw sums of
//                                         k_field_grid's arena, field by field: S, SP, Sρ, Sv[3], n — 7 × nodes doubles
//                                    OUT: int64 nv, ne, dims; double vertices[nv × 3]; int32 elements[ne × dims];
//                                         double pressure[nv]; double velocity[nv × 3]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sphmi_iso_core.h"

using namespace sphmi;

template <int D> static void print_table() {
    const IsoTable<D>& T = iso_table<D>();
    for (int s = 0; s < T.kSimplices; ++s)
        for (int set = 0; set < T.kSets; ++set) {
            printf("%d %d ", D, s);
            for (int k = 0; k < D; ++k) printf("%d", (int)T.perm[s][k]);
            printf(" %d %d %d", set, (int)T.count[s][set], (int)T.swapped[s][set]);
            for (int e = 0; e < T.count[s][set]; ++e)
                for (int v = 0; v < D; ++v) printf(" %d:%d", T.vertex[s][set][e][v] >> 3, T.vertex[s][set][e][v] & 7);
            printf("\n");
        }
}

static bool read_exact(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }
static bool write_exact(FILE* f, const void* p, size_t bytes) { return bytes == 0 || fwrite(p, 1, bytes, f) == bytes; }

template <int D> static void extract(IsoArgs& A, std::vector<double>& vertices, std::vector<int>& elements, std::vector<double>& pressure, std::vector<double>& velocity) {
    const size_t n = (size_t)A.nodes;
    std::vector<unsigned char> mask(n), corners(n);
    std::vector<int> vcount(n), ecount(n);
    std::vector<long long> voff(n + 1, 0), eoff(n + 1, 0);
    A.mask = mask.data(); A.corners = corners.data(); A.vcount = vcount.data(); A.ecount = ecount.data();
    for (int k = 0; k < A.nodes; ++k) iso_classify_node<D>(A, k);
    for (size_t k = 0; k < n; ++k) { voff[k + 1] = voff[k] + vcount[k]; eoff[k + 1] = eoff[k] + ecount[k]; }
    A.voff = voff.data(); A.eoff = eoff.data();
    vertices.assign((size_t)voff[n] * 3, -1.0); pressure.assign((size_t)voff[n], -1.0); velocity.assign((size_t)voff[n] * 3, -1.0);
    elements.assign((size_t)eoff[n] * D, -1);
    A.vertices = vertices.data(); A.pressure = pressure.data(); A.velocity = velocity.data(); A.elements = elements.data();
    for (int k = 0; k < A.nodes; ++k) iso_node_vertices<D>(A, k);
    for (int k = 0; k < A.nodes; ++k) iso_cell_elements<D>(A, k);
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "--table")) { print_table<2>(); print_table<3>(); return 0; }
    if (argc != 3) { fprintf(stderr, "usage: iso_main --table | iso_main IN OUT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { fprintf(stderr, "iso_main: cannot open %s\n", argv[1]); return 2; }
    int64_t dims = 0, counts[3] = {1, 1, 1};
    IsoArgs A{};
    bool ok = read_exact(in, &dims, 8) && read_exact(in, counts, 24) && read_exact(in, A.origin, 24) && read_exact(in, A.spacing, 24) && read_exact(in, &A.level, 8);
    if (!ok || (dims != 2 && dims != 3)) { fprintf(stderr, "iso_main: bad header\n"); return 2; }
    int64_t nodes = 1;
    for (int d = 0; d < 3; ++d) {
        if (d >= dims) counts[d] = 1;
        if (counts[d] < 1 || counts[d] > (1 << 24) || nodes * counts[d] > (1 << 24)) { fprintf(stderr, "iso_main: bad counts\n"); return 2; }
        nodes *= counts[d];
        A.counts[d] = (int)counts[d];
    }
    A.nodes = (int)nodes;
    std::vector<double> sums((size_t)7 * (size_t)nodes);
    ok = read_exact(in, sums.data(), sums.size() * 8);
    fclose(in);
    if (!ok) { fprintf(stderr, "iso_main: short file\n"); return 2; }
    A.sums = sums.data();
    std::vector<double> vertices, pressure, velocity;
    std::vector<int> elements;
    if (dims == 3) extract<3>(A, vertices, elements, pressure, velocity);
    else extract<2>(A, vertices, elements, pressure, velocity);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { fprintf(stderr, "iso_main: cannot open %s\n", argv[2]); return 2; }
    const int64_t head[3] = {(int64_t)pressure.size(), (int64_t)(elements.size() / (size_t)dims), dims};
    ok = write_exact(out, head, 24) && write_exact(out, vertices.data(), vertices.size() * 8) && write_exact(out, elements.data(), elements.size() * 4) &&
         write_exact(out, pressure.data(), pressure.size() * 8) && write_exact(out, velocity.data(), velocity.size() * 8);
    ok = fclose(out) == 0 && ok;
    if (!ok) { fprintf(stderr, "iso_main: write failed\n"); return 2; }
    printf("%lld vertices, %lld elements\nok\n", (long long)head[0], (long long)head[1]);
    return 0;
}
