// The plan of the point-cloud sampler (sphexample_amd/csrc/sphmi_point_cloud.h: pc_tiling, pc_blocks, pc_plan_point, pc_plan_tiles;
// sphmi_series.h: check_sample_points) compiled for the host: built with the host compiler and the address / undefined-behaviour
// sanitizers by tests/test_sample_points_host.py, run as a child process.
//
//     points_main               the self checks
//     points_main IN OUT        … and a cloud: IN holds a cell grid and points, OUT receives the bins, which the test compares with a
//                               numpy restatement
// IN, every item 8 bytes: gmin[3], np[3], dims, n (int64), H_inv (double), then n rows of `dims` doubles.
// OUT, int64 throughout: blocks, tiles in all, cell[n][3], block[n], slot[n] — the place of point p in the index array when every
// block hands out its slots in the caller's order — points[blocks], tiles[blocks], then per tile { first, count }.
// Exit code 0 and "ok" on the last line: every check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "sphmi_point_cloud.h"

using namespace sphmi;

static int g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity();
static const double kNaN = std::numeric_limits<double>::quiet_NaN();

static std::string refusal(int64_t n, const double* x, int dims) {
    try { check_sample_points(n, x, dims); }
    catch (const EngineError& e) { return e.status == SPHMI_ERR_ARGUMENT ? e.what() : "another status"; }
    return "";
}

static void test_argument_check() {
    CHECK(kMaxSamplePoints == SPHMI_MAX_SAMPLE_POINTS && kPcTile == 256);
    const double x[6] = {0.0, 1.0, 2.0, -1e300, 5e-324, 7.0};
    CHECK(refusal(0, nullptr, 3).empty() && refusal(0, x, 2).empty() && refusal(2, x, 3).empty() && refusal(3, x, 2).empty());
    CHECK(refusal(1, nullptr, 2).find("null positions") != std::string::npos);
    CHECK(refusal(-1, x, 2).find("n_points") != std::string::npos && refusal(kMaxSamplePoints + 1, nullptr, 2).find("n_points") != std::string::npos);
    const double bad[6] = {0.0, 1.0, 2.0, 3.0, kNaN, kInf};
    CHECK(refusal(3, bad, 2).find("at point 2") != std::string::npos);      // 2-D: the NaN is coordinate 0 of point 2
    CHECK(refusal(2, bad, 3).find("at point 1") != std::string::npos);      // 3-D: coordinate 1 of point 1
    CHECK(refusal(2, bad, 2).empty());                                      // the first two points are finite
    const double neg[2] = {0.0, -kInf};
    CHECK(refusal(1, neg, 2).find("at point 0") != std::string::npos);
}

static void test_plan() {
    CHECK(pc_block_cells(3) == 3 && pc_block_cells(2) == 6);
    CHECK(pc_plan_tiles(0) == 0 && pc_plan_tiles(1) == 1 && pc_plan_tiles(256) == 1 && pc_plan_tiles(257) == 2 && pc_plan_tiles(513) == 3);
    // cells −2 … 9 per axis (np = 14: padded index 1 is cell −2), H = 0.5
    const int gmin[3] = {-2, -2, -2}, np[3] = {14, 8, 7};
    const PcTiling G = pc_tiling(gmin, np, 3, 2.0);
    CHECK(G.B == 3 && G.nb[0] == 5 && G.nb[1] == 3 && G.nb[2] == 3 && pc_blocks(G) == 45);
    const double at0[3] = {0.0, 0.0, 0.0};
    PcPlan P = pc_plan_point(G, at0);
    CHECK(P.cell[0] == 3 && P.cell[1] == 3 && P.cell[2] == 3 && P.block == 1 + 5 * (1 + 3 * 1));
    // a face: cell c covers |x/H − c| ≤ ½, the half goes away from zero
    const double face[3] = {0.25, -0.25, 0.2499999999999999};
    P = pc_plan_point(G, face);
    CHECK(P.cell[0] == 4 && P.cell[1] == 2 && P.cell[2] == 3);
    // outside on every side, by a little and by everything a double holds: the outermost cell, the outermost block
    const double below[3] = {-1.6, -1e300, -1.7976931348623157e308}, above[3] = {6.0, 1e300, 1.7976931348623157e308};
    P = pc_plan_point(G, below);
    CHECK(P.cell[0] == 0 && P.cell[1] == 0 && P.cell[2] == 0 && P.block == 0);
    P = pc_plan_point(G, above);
    CHECK(P.cell[0] == 13 && P.cell[1] == 7 && P.cell[2] == 6 && P.block == 44);
    // 2-D: the third axis is one cell, one block, whatever lies behind x[1]
    const PcTiling G2 = pc_tiling(gmin, np, 2, 2.0);
    CHECK(G2.B == 6 && G2.nb[0] == 3 && G2.nb[1] == 2 && G2.nb[2] == 1 && G2.np[2] == 1 && pc_blocks(G2) == 6);
    const double p2[2] = {3.1, 0.9};
    P = pc_plan_point(G2, p2);
    CHECK(P.cell[0] == 9 && P.cell[1] == 5 && P.cell[2] == 0 && P.block == 1);
}

static void run_case(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    CHECK(f != nullptr);
    auto rd = [&](void* p, size_t n) { CHECK(fread(p, 8, n, f) == n); };
    int64_t g[8];
    double H_inv;
    rd(g, 8); rd(&H_inv, 1);
    const int gmin[3] = {(int)g[0], (int)g[1], (int)g[2]}, np[3] = {(int)g[3], (int)g[4], (int)g[5]};
    const int dims = (int)g[6];
    const int64_t n = g[7];
    CHECK((dims == 2 || dims == 3) && n >= 0);
    std::vector<double> x((size_t)n * dims);
    if (n) rd(x.data(), x.size());
    fclose(f);
    check_sample_points(n, x.data(), dims);
    const PcTiling G = pc_tiling(gmin, np, dims, H_inv);
    const int64_t blocks = pc_blocks(G);
    std::vector<int64_t> cell((size_t)n * 3), block((size_t)n), slot((size_t)n), points((size_t)blocks, 0), tiles((size_t)blocks), first((size_t)blocks + 1, 0);
    for (int64_t p = 0; p < n; ++p) {
        const PcPlan P = pc_plan_point(G, &x[(size_t)p * dims]);
        CHECK(P.block >= 0 && P.block < blocks);
        for (int d = 0; d < 3; ++d) { CHECK(P.cell[d] >= 0 && P.cell[d] < G.np[d]); cell[(size_t)p * 3 + d] = P.cell[d]; }
        block[(size_t)p] = P.block;
        slot[(size_t)p] = points[(size_t)P.block]++;                    // the rank within the block for now
    }
    int64_t total = 0;
    for (int64_t b = 0; b < blocks; ++b) {
        tiles[(size_t)b] = pc_plan_tiles((int)points[(size_t)b]);
        first[(size_t)b + 1] = first[(size_t)b] + points[(size_t)b];
        total += tiles[(size_t)b];
    }
    CHECK(first[(size_t)blocks] == n);
    for (int64_t p = 0; p < n; ++p) slot[(size_t)p] += first[(size_t)block[(size_t)p]];
    std::vector<int64_t> desc;
    for (int64_t b = 0; b < blocks; ++b)
        for (int64_t k = 0; k < tiles[(size_t)b]; ++k) {
            desc.push_back(first[(size_t)b] + kPcTile * k);
            desc.push_back(std::min<int64_t>(kPcTile, points[(size_t)b] - kPcTile * k));
        }
    CHECK((int64_t)desc.size() == 2 * total);
    FILE* o = fopen(out_path, "wb");
    CHECK(o != nullptr);
    auto wr = [&](const void* p, size_t m) { if (m) CHECK(fwrite(p, 8, m, o) == m); };
    wr(&blocks, 1); wr(&total, 1);
    wr(cell.data(), cell.size()); wr(block.data(), block.size()); wr(slot.data(), slot.size());
    wr(points.data(), points.size()); wr(tiles.data(), tiles.size()); wr(desc.data(), desc.size());
    CHECK(fclose(o) == 0);
}

int main(int argc, char** argv) {
    test_argument_check();
    test_plan();
    if (argc == 3) run_case(argv[1], argv[2]);
    printf("%d checks\nok\n", g_checks);
    return 0;
}
