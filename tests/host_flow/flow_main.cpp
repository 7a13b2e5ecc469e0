// The host side of the flow through control boxes (sphexample_amd/csrc/sphmi_series.h: check_flow_table, deliver_flow, and the
// StepSeries a read goes through) on hand-made tables and records: built with the host compiler and the address /
// undefined-behaviour sanitizers by tests/test_flow_host.py, run as a child process.  Exit code 0 and "ok" on the last line: every
// check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "sphmi_series.h"

using namespace sphmi;

static int g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static const char* kFn = "sphmi_flow_read";
static const double kInf = std::numeric_limits<double>::infinity();
static const double kNaN = std::numeric_limits<double>::quiet_NaN();

// does check_flow_table refuse the table, with SPHMI_ERR_ARGUMENT and this text?
static bool refused(int32_t n, const double* lo, const double* hi, int dims, int64_t cap, const char* text) {
    try { check_flow_table(n, lo, hi, dims, cap); }
    catch (const EngineError& e) { return e.status == SPHMI_ERR_ARGUMENT && std::string(e.what()) == std::string("sphmi_flow_enable: ") + text; }
    return false;
}
static bool accepted(int32_t n, const double* lo, const double* hi, int dims, int64_t cap) {
    try { check_flow_table(n, lo, hi, dims, cap); } catch (const EngineError&) { return false; }
    return true;
}

static void test_table() {
    CHECK(kMaxFlowBoxes == 16 && kMaxFlowBoxes == SPHMI_MAX_FLOW_BOXES && kFlValues == 7);
    // exactly n × dims bounds: the sanitizer sees a read past them
    for (int dims = 2; dims <= 3; ++dims) {
        std::vector<double> lo((size_t)2 * dims, 0.0), hi((size_t)2 * dims, 1.0);
        CHECK(accepted(2, lo.data(), hi.data(), dims, 1));
        // ±inf are bounds like any other, on one side or on both
        lo[0] = -kInf; hi[(size_t)dims] = kInf; lo[(size_t)dims + 1] = -kInf; hi[(size_t)dims + 1] = kInf;
        CHECK(accepted(2, lo.data(), hi.data(), dims, 1));
        // a NaN bound on either side, in the last box's last axis too
        for (size_t at : {(size_t)0, (size_t)2 * dims - 1}) {
            std::vector<double> l = lo, h = hi;
            l[at] = kNaN;
            CHECK(refused(2, l.data(), h.data(), dims, 1, "NaN bound"));
            l = lo; h[at] = kNaN;
            CHECK(refused(2, l.data(), h.data(), dims, 1, "NaN bound"));
        }
        // lo == hi and lo > hi on any axis; (-inf, -inf) and (+inf, +inf) hold no row either
        for (size_t at = 0; at < (size_t)2 * dims; ++at) {
            std::vector<double> l = lo, h = hi;
            l[at] = 0.25; h[at] = 0.25;
            CHECK(refused(2, l.data(), h.data(), dims, 1, "every box needs lo < hi on every axis"));
            h[at] = 0.125;
            CHECK(refused(2, l.data(), h.data(), dims, 1, "every box needs lo < hi on every axis"));
            l[at] = -kInf; h[at] = -kInf;
            CHECK(refused(2, l.data(), h.data(), dims, 1, "every box needs lo < hi on every axis"));
            l[at] = kInf; h[at] = kInf;
            CHECK(refused(2, l.data(), h.data(), dims, 1, "every box needs lo < hi on every axis"));
        }
        // the number of boxes
        std::vector<double> l16((size_t)16 * dims, -1.0), h16((size_t)16 * dims, 1.0);
        CHECK(accepted(16, l16.data(), h16.data(), dims, 1));
        CHECK(refused(17, l16.data(), h16.data(), dims, 1, "n_boxes out of range [0, 16]"));
        CHECK(refused(-1, l16.data(), h16.data(), dims, 1, "n_boxes out of range [0, 16]"));
        // null tables, the capacity
        CHECK(refused(1, nullptr, h16.data(), dims, 1, "null table"));
        CHECK(refused(1, l16.data(), nullptr, dims, 1, "null table"));
        CHECK(refused(1, l16.data(), h16.data(), dims, 0, "capacity_steps must be positive"));
        CHECK(refused(1, l16.data(), h16.data(), dims, -3, "capacity_steps must be positive"));
        // n_boxes = 0 disables: nothing else is looked at
        CHECK(accepted(0, nullptr, nullptr, dims, 0));
    }
}

// a record of `n_boxes` boxes: slot c of box b holds base + 10 b + c, the three counts whole numbers
static std::vector<double> record(int64_t it, int n_boxes, double base) {
    std::vector<double> r((size_t)kStepHeader + (size_t)kFlValues * n_boxes, 0.0);
    memcpy(&r[0], &it, 8);
    r[1] = 0.5 * (double)it; r[2] = 0.125;
    for (int b = 0; b < n_boxes; ++b)
        for (int c = 0; c < kFlValues; ++c) r[(size_t)kStepHeader + (size_t)kFlValues * b + c] = base + 10.0 * b + c + (c >= 1 && c <= 4 ? 0.5 : 0.0);
    return r;
}

// the arrays of one read, exactly `cap` samples long (the sanitizer sees a write past them)
struct Got {
    std::vector<int64_t> it, count, entered, left;
    std::vector<double> t, dt, volume, momentum;
    int64_t n = -7, dropped = -7;
    Got(int64_t cap, int m)
        : it((size_t)cap, -1), count((size_t)cap * m, -1), entered((size_t)cap * m, -1), left((size_t)cap * m, -1), t((size_t)cap, -1.0), dt((size_t)cap, -1.0),
          volume((size_t)cap * m, -1.0), momentum((size_t)cap * m * 3, -1.0) {}
};
static Got read(StepSeries& s, double m0, int m, int64_t cap) {
    Got g(cap, m);
    s.read(kFn, cap, g.it.data(), g.t.data(), g.dt.data(), &g.n, &g.dropped, [&](int64_t k, const double* v) {
        deliver_flow(m0, m, k, v, g.count.data(), g.volume.data(), g.momentum.data(), g.entered.data(), g.left.data());
    });
    return g;
}

static void test_delivery() {
    const double m0 = 0.008;
    const int m = 3;
    StepSeries s;
    s.reset(kFlValues * m, 4);
    const std::vector<double> r1 = record(3, m, 100.0), r2 = record(4, m, 200.0);
    s.push(StepSeries::decode(r1.data(), kStepHeader, kFlValues * m));
    s.push(StepSeries::decode(r2.data(), kStepHeader, kFlValues * m));
    Got got = read(s, m0, m, 2);
    CHECK(got.n == 2 && got.dropped == 0 && got.it[0] == 3 && got.it[1] == 4 && got.t[0] == 1.5 && got.dt[1] == 0.125);
    for (int k = 0; k < 2; ++k)
        for (int b = 0; b < m; ++b) {
            const double* v = (k == 0 ? r1 : r2).data() + kStepHeader + kFlValues * b;
            const size_t at = (size_t)k * m + b;
            CHECK(got.count[at] == (int64_t)v[0] && got.entered[at] == (int64_t)v[5] && got.left[at] == (int64_t)v[6]);
            CHECK(got.volume[at] == m0 * v[1]);                      // one multiplication each
            for (int d = 0; d < 3; ++d) CHECK(got.momentum[3 * at + d] == m0 * v[2 + d]);
        }
    CHECK(got.count[0] == 100 && got.entered[0] == 105 && got.left[0] == 106 && got.count[(size_t)m + 2] == 220);
    // every output null: the samples still leave the series
    s.push(StepSeries::decode(r1.data(), kStepHeader, kFlValues * m));
    int64_t n = -1;
    s.read(kFn, 1, nullptr, nullptr, nullptr, &n, nullptr, [&](int64_t k, const double* p) { deliver_flow(m0, m, k, p, nullptr, nullptr, nullptr, nullptr, nullptr); });
    CHECK(n == 1 && s.q.empty());
    // two slabs' records of a step add slot by slot; records of different steps do not
    StepSeries::Sample a = StepSeries::decode(r1.data(), kStepHeader, kFlValues * m);
    const StepSeries::Sample a0 = a, b = StepSeries::decode(record(3, m, 1.0).data(), kStepHeader, kFlValues * m);
    StepSeries::add(a, b, "flow");
    for (size_t c = 0; c < a.v.size(); ++c) CHECK(a.v[c] == a0.v[c] + b.v[c]);
    try { StepSeries::add(a, StepSeries::decode(r2.data(), kStepHeader, kFlValues * m), "flow"); CHECK(false); }
    catch (const EngineError& err) { CHECK(err.status == SPHMI_ERR_STATE && std::string(err.what()) == "flow: the slabs' records of a step do not belong together"); }
}

// a read with capacity = 0 clears nothing; samples beyond capacity_steps are dropped and counted
static void test_capacity() {
    const int m = 16;
    StepSeries s;
    s.reset(kFlValues * m, 6);
    for (int64_t it = 1; it <= 50; ++it) s.push(StepSeries::decode(record(it, m, (double)(1000 * it)).data(), kStepHeader, kFlValues * m));
    for (int rep = 0; rep < 2; ++rep) {
        int64_t n = -1, d = -1;
        s.read(kFn, 0, nullptr, nullptr, nullptr, &n, &d, [&](int64_t, const double*) { CHECK(false); });
        CHECK(n == 6 && d == 44 && s.q.size() == 6 && s.dropped == 44);
    }
    Got got = read(s, 1.0, m, 7);
    CHECK(got.n == 6 && got.dropped == 44);
    for (int64_t k = 0; k < 6; ++k) {
        CHECK(got.it[(size_t)k] == 45 + k && got.count[(size_t)k * m] == 1000 * (45 + k) && got.left[(size_t)k * m + 15] == 1000 * (45 + k) + 156);
        CHECK(got.volume[(size_t)k * m + 1] == (double)(1000 * (45 + k)) + 11.5);
    }
    CHECK(got.it[6] == -1 && got.count[(size_t)6 * m] == -1 && got.momentum[(size_t)6 * m * 3] == -1.0);      // nothing behind the delivered ones
    got = read(s, 1.0, m, 7);
    CHECK(got.n == 0 && got.dropped == 0);
    // a partial read leaves the rest, and the dropped count is handed out once
    for (int64_t it = 1; it <= 8; ++it) s.push(StepSeries::decode(record(it, m, 0.0).data(), kStepHeader, kFlValues * m));
    got = read(s, 1.0, m, 4);
    CHECK(got.n == 4 && got.dropped == 2 && got.it[0] == 3 && got.it[3] == 6);
    got = read(s, 1.0, m, 4);
    CHECK(got.n == 2 && got.dropped == 0 && got.it[0] == 7 && got.it[1] == 8 && got.it[2] == -1);
    // the argument errors are the series' own
    int64_t n = -1;
    try { s.read(kFn, 1, nullptr, nullptr, nullptr, nullptr, nullptr, [&](int64_t, const double*) {}); CHECK(false); }
    catch (const EngineError& err) { CHECK(err.status == SPHMI_ERR_ARGUMENT && std::string(err.what()) == "sphmi_flow_read: null n_out"); }
    try { s.read(kFn, -1, nullptr, nullptr, nullptr, &n, nullptr, [&](int64_t, const double*) {}); CHECK(false); }
    catch (const EngineError& err) { CHECK(err.status == SPHMI_ERR_ARGUMENT && std::string(err.what()) == "sphmi_flow_read: negative capacity"); }
}

int main() {
    test_table();
    test_delivery();
    test_capacity();
    printf("%d checks\nok\n", g_checks);
    return 0;
}
