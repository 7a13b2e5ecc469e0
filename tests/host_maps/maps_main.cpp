// The index, image and record arithmetic of the per-bin maps (sphexample_amd/csrc/sphmi_maps.h: mp_bin, mp_image / mp_value, mp_fixed /
// mp_unfixed, mp_fold; sphmi_series.h: check_map_lattice, map_row_bound, deliver_map_vectors) compiled for the host: built with the
// host compiler and the address / undefined-behaviour sanitizers by tests/test_maps_host.py, run as a child process.
//
//     maps_main                 the self checks
//     maps_main IN OUT          … and a dumped case: IN holds a lattice and the rows of some steps, OUT receives the records, the
//                               window and the map of the last step, which the test compares with sphexample_amd.maps.update
// IN, every item 8 bytes: origin[3], spacing[3] (double), counts[3], up, t_begin (double), steps (int64), then per step t, dt (double),
// n (int64) and n rows of { x, y, z, vx, vy, vz, fluid (0.0 / 1.0) }.  OUT: kMpValues arrays of `bins` doubles, { steps (int64), t_begin,
// t_end, duration }, then last n (int64) [bins], top [bins], bottom [bins], Sd [bins][3].
// Exit code 0 and "ok" on the last line: every check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "sphmi_maps.h"

using namespace sphmi;

static int g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static const double kInf = std::numeric_limits<double>::infinity();
static const double kNaN = std::numeric_limits<double>::quiet_NaN();

static bool refused(const double* o, const double* s, const int64_t* c, int dims, int up) {
    try { check_map_lattice(o, s, c, dims, up); }
    catch (const EngineError& e) { return e.status == SPHMI_ERR_ARGUMENT && std::string(e.what()).rfind("sphmi_maps_enable: ", 0) == 0; }
    return false;
}

static void test_lattice_check() {
    CHECK(kMpValues == 12 && kMpHeader == 4 && kMaxMapBins == SPHMI_MAX_MAP_BINS);
    const double o[3] = {0.0, -1.0, 2.0}, s[3] = {0.5, 0.25, kInf};
    const int64_t c[3] = {4, 8, 1};
    CHECK(check_map_lattice(o, s, c, 3, 2) == 32 && check_map_lattice(o, s, c, 2, 1) == 32);
    CHECK(refused(nullptr, s, c, 3, 0) && refused(o, nullptr, c, 3, 0) && refused(o, s, nullptr, 3, 0));
    CHECK(refused(o, s, c, 3, 3) && refused(o, s, c, 3, -1) && refused(o, s, c, 2, 2));
    const double o_nan[3] = {0.0, kNaN, 0.0}, o_inf[3] = {kInf, 0.0, 0.0};
    CHECK(refused(o_nan, s, c, 3, 0) && refused(o_inf, s, c, 3, 0));
    const double s_zero[3] = {0.0, 0.25, kInf}, s_neg[3] = {0.5, -0.25, kInf}, s_nan[3] = {0.5, kNaN, kInf}, s_ninf[3] = {0.5, 0.25, -kInf};
    CHECK(refused(o, s_zero, c, 3, 0) && refused(o, s_neg, c, 3, 0) && refused(o, s_nan, c, 3, 0) && refused(o, s_ninf, c, 3, 0));
    const int64_t c_two[3] = {4, 8, 2}, c_zero[3] = {4, 0, 1}, c_big[3] = {1 << 10, (1 << 10) + 1, 1}, c_huge[3] = {int64_t(1) << 40, int64_t(1) << 40, 1};
    CHECK(refused(o, s, c_two, 3, 0));                   // +inf spacing with a count above 1
    CHECK(refused(o, s, c_zero, 3, 0) && refused(o, s, c_big, 3, 0) && refused(o, s, c_huge, 3, 0));
    const int64_t c_limit[3] = {1 << 10, 1 << 10, 1};
    CHECK(check_map_lattice(o, s, c_limit, 3, 0) == SPHMI_MAX_MAP_BINS);
    CHECK(map_row_bound(20.0) == 26843545 && map_row_bound(0.0) == INT64_MAX && map_row_bound(1e-300) == INT64_MAX);
}

static void test_images() {
    const double v[] = {-kInf, -1e300, -2.5, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 2.5, 1e300, kInf};
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int k = 0; k < n; ++k) {
        const double back = mp_value(mp_image(v[k]));
        CHECK(memcmp(&back, &v[k], 8) == 0);
        if (k) CHECK(mp_image(v[k - 1]) < mp_image(v[k]));          // strictly: −0 lies below +0
        CHECK(mp_image(v[k]) > kMpTopIdentity && mp_image(v[k]) < kMpBottomIdentity);
    }
    // the fixed-point velocity: half to even, exact powers of two, the sign
    CHECK(mp_fixed(1.0) == (1ll << 32) && mp_fixed(-1.0) == -(1ll << 32) && mp_fixed(0.0) == 0 && mp_fixed(-0.0) == 0);
    CHECK(mp_fixed(0.5 / 4294967296.0) == 0 && mp_fixed(1.5 / 4294967296.0) == 2 && mp_fixed(2.5 / 4294967296.0) == 2 && mp_fixed(-0.5 / 4294967296.0) == 0);
    CHECK(mp_unfixed(1ll << 32) == 1.0 && mp_unfixed(-3) == -3.0 / 4294967296.0 && mp_unfixed((1ll << 62) + 1) == 1073741824.0);
    CHECK(mp_finite(0.0) && mp_finite(-1e308) && !mp_finite(kInf) && !mp_finite(-kInf) && !mp_finite(kNaN));
}

static void test_bins() {
    MapLattice L{};
    const double o[3] = {0.25, -1.0, 0.0}, s[3] = {0.5, 0.25, kInf};
    const int c[3] = {4, 8, 1};
    for (int d = 0; d < 3; ++d) { L.origin[d] = o[d]; L.spacing[d] = s[d]; L.counts[d] = c[d]; L.countd[d] = (double)c[d]; }
    L.up = 2; L.bins = 32;
    CHECK(mp_bin(L, 0.25, -1.0, 0.0) == 0);                         // on the lower faces: inside
    CHECK(mp_bin(L, 0.75, -1.0, 5.0) == 1 && mp_bin(L, 0.7499999999999999, -1.0, 5.0) == 0);      // an inner edge belongs to the upper bin
    CHECK(mp_bin(L, 2.25, -1.0, 0.0) == -1 && mp_bin(L, 0.25, 1.0, 0.0) == -1);                   // the upper faces: outside
    CHECK(mp_bin(L, 2.2499999999999996, 0.99, 0.0) == 31);
    CHECK(mp_bin(L, 0.2499999999999999, 0.0, 0.0) == -1);
    CHECK(mp_bin(L, 1.0, 0.0, -7.0) == 1 + 4 * 4 && mp_bin(L, 1.0, 0.0, -1e300) == 17);           // below the origin of a collapsed axis: −0, inside
    CHECK(mp_bin(L, kNaN, 0.0, 0.0) == -1 && mp_bin(L, 1.0, kNaN, 0.0) == -1 && mp_bin(L, 1.0, 0.0, kNaN) == -1);
    CHECK(mp_bin(L, 1.0, 0.0, kInf) == -1 && mp_bin(L, 1.0, 0.0, -kInf) == -1 && mp_bin(L, kInf, 0.0, 0.0) == -1 && mp_bin(L, -kInf, 0.0, 0.0) == -1);
    CHECK(mp_bin(L, 1e300, 0.0, 0.0) == -1 && mp_bin(L, -1e300, 0.0, 0.0) == -1);
}

static void test_fold() {
    std::vector<double> r(kMpValues);
    for (int k = 0; k < kMpValues; ++k) r[k] = mp_start(k);
    CHECK(r[0] == -kInf && r[1] == 0.0 && r[2] == kInf && r[3] == kInf && r[4] == 0.0 && r[9] == 0.0 && r[11] == 0.0);
    const long long S[3] = {3ll << 32, -(4ll << 32), 0};
    mp_fold(r.data(), 1, 2, mp_image(0.5), mp_image(-0.0), S, 1.5, 0.25);
    CHECK(r[0] == 0.5 && r[1] == 1.5 && r[2] == 0.0 && std::signbit(r[2]) && r[3] == 1.5 && r[4] == 0.25 && r[5] == 0.5);
    CHECK(r[6] == 0.75 && r[7] == -1.0 && r[8] == 0.0 && r[9] == 1.5 * 1.5 + 2.0 * 2.0 && r[10] == 1.5 && r[11] == 2.0);
    // the same crest again: the first attainment keeps its time; a slower, emptier step moves only the sums
    const long long S2[3] = {1ll << 32, 0, 0};
    mp_fold(r.data(), 1, 1, mp_image(0.5), mp_image(0.25), S2, 2.0, 0.5);
    CHECK(r[0] == 0.5 && r[1] == 1.5 && r[2] == 0.0 && r[3] == 1.5 && r[4] == 0.75 && r[5] == 1.0 && r[6] == 1.25 && r[9] == 6.25 && r[10] == 1.5 && r[11] == 2.0);
    // a stride: the slots of one bin among those of others (exactly kMpValues · stride doubles: the sanitizer sees a step past them)
    std::vector<double> q(kMpValues * 3, kNaN);
    for (int k = 0; k < kMpValues; ++k) q[3 * k + 2] = mp_start(k);
    mp_fold(q.data() + 2, 3, 2, mp_image(0.5), mp_image(-0.0), S, 1.5, 0.25);
    for (int k = 0; k < kMpValues; ++k) CHECK(std::isnan(q[3 * k]) && std::isnan(q[3 * k + 1]));
    CHECK(q[2] == 0.5 && q[3 * 11 + 2] == 2.0 && q[3 * 7 + 2] == -1.0);
    double out[6] = {0};
    const double c0[2] = {1, 2}, c1[2] = {3, 4}, c2[2] = {5, 6};
    deliver_map_vectors(2, c0, c1, c2, out);
    CHECK(out[0] == 1 && out[1] == 3 && out[2] == 5 && out[3] == 2 && out[4] == 4 && out[5] == 6);
    deliver_map_vectors(2, c0, c1, c2, nullptr);
}

static void run_case(const char* in_path, const char* out_path) {
    FILE* f = fopen(in_path, "rb");
    CHECK(f != nullptr);
    auto rd = [&](void* p, size_t n) { CHECK(fread(p, 8, n, f) == n); };
    MapLattice L{};
    int64_t counts[3], up, steps;
    double t_begin;
    rd(L.origin, 3); rd(L.spacing, 3); rd(counts, 3); rd(&up, 1); rd(&t_begin, 1); rd(&steps, 1);
    CHECK(check_map_lattice(L.origin, L.spacing, counts, 3, (int32_t)up) == counts[0] * counts[1] * counts[2]);
    for (int d = 0; d < 3; ++d) { L.counts[d] = (int)counts[d]; L.countd[d] = (double)counts[d]; }
    L.up = (int)up; L.bins = (int)(counts[0] * counts[1] * counts[2]);
    const size_t B = (size_t)L.bins;
    std::vector<double> rec(kMpValues * B);
    for (int k = 0; k < kMpValues; ++k) for (size_t b = 0; b < B; ++b) rec[k * B + b] = mp_start(k);
    double header[kMpHeader] = {0.0, t_begin, t_begin, 0.0};
    std::vector<uint32_t> n(B);
    std::vector<uint64_t> top(B), bottom(B);
    std::vector<long long> S(3 * B);
    for (int64_t k = 0; k < steps; ++k) {
        double t, dt;
        int64_t rows;
        rd(&t, 1); rd(&dt, 1); rd(&rows, 1);
        std::vector<double> row((size_t)rows * 7);
        if (rows) rd(row.data(), row.size());
        n.assign(B, 0u); top.assign(B, kMpTopIdentity); bottom.assign(B, kMpBottomIdentity); S.assign(3 * B, 0ll);
        for (int64_t i = 0; i < rows; ++i) {
            const double* q = &row[(size_t)i * 7];
            if (q[6] == 0.0 || !mp_finite(q[3]) || !mp_finite(q[4]) || !mp_finite(q[5])) continue;
            const int b = mp_bin(L, q[0], q[1], q[2]);
            if (b < 0) continue;
            CHECK((size_t)b < B);
            const uint64_t im = mp_image(q[L.up]);
            n[b] += 1u;
            if (im > top[b]) top[b] = im;
            if (im < bottom[b]) bottom[b] = im;
            for (int d = 0; d < 3; ++d) S[3 * b + d] += mp_fixed(q[3 + d]);
        }
        for (size_t b = 0; b < B; ++b) if (n[b]) mp_fold(&rec[b], B, n[b], top[b], bottom[b], &S[3 * b], t, dt);
        int64_t done;
        memcpy(&done, &header[0], 8);
        done += 1;
        memcpy(&header[0], &done, 8);
        header[2] = t;
        header[3] = header[3] + dt;
    }
    fclose(f);
    FILE* g = fopen(out_path, "wb");
    CHECK(g != nullptr);
    auto wr = [&](const void* p, size_t m) { CHECK(fwrite(p, 8, m, g) == m); };
    wr(rec.data(), rec.size());
    wr(header, kMpHeader);
    std::vector<int64_t> ln(B);
    std::vector<double> lt(B), lb(B), ls(3 * B);
    for (size_t b = 0; b < B; ++b) {
        ln[b] = n[b];
        lt[b] = n[b] ? mp_value(top[b]) : mp_start(0);
        lb[b] = n[b] ? mp_value(bottom[b]) : mp_start(2);
        for (int d = 0; d < 3; ++d) ls[3 * b + d] = mp_unfixed(S[3 * b + d]);
    }
    wr(ln.data(), B); wr(lt.data(), B); wr(lb.data(), B); wr(ls.data(), 3 * B);
    CHECK(fclose(g) == 0);
}

int main(int argc, char** argv) {
    test_lattice_check();
    test_images();
    test_bins();
    test_fold();
    if (argc == 3) run_case(argv[1], argv[2]);
    printf("%d checks\nok\n", g_checks);
    return 0;
}
