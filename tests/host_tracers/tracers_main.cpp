// The host side of the tracers (sphexample_amd/csrc/sphmi_series.h: check_tracer_table, deliver_tracers) on hand-made tables and
// records: built with the host compiler and the address / undefined-behaviour sanitizers by tests/test_tracers_host.py, run as a
// child process.  Exit code 0 and "ok" on the last line: every check held.
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

static const double kInf = std::numeric_limits<double>::infinity();
static const double kNaN = std::numeric_limits<double>::quiet_NaN();

// 0: accepted; 1: refused with SPHMI_ERR_ARGUMENT and the prefix; 2: refused some other way
static int verdict(int32_t np, const int64_t* rows, int64_t n_rows, int32_t nd, const double* pos, int dims, double min_weight, int64_t cap) {
    try { check_tracer_table(np, rows, n_rows, nd, pos, dims, min_weight, cap); }
    catch (const EngineError& e) { return e.status == SPHMI_ERR_ARGUMENT && std::string(e.what()).rfind("sphmi_tracers_enable: ", 0) == 0 ? 1 : 2; }
    return 0;
}

static void test_table() {
    CHECK(kMaxTracers == SPHMI_MAX_TRACERS && kMaxTracers == 1024 && kTrParticleValues == 8 && kTrDrifterValues == 10 && kTrDrifterValues == 3 + kPrValues);
    const int64_t rows[4] = {7, 0, 99, 3};
    const double pos[6] = {0.1, 0.2, 0.3, -4.0, 5.0, 1e300};
    // accepted: both kinds, either alone, one of each, 2-D and 3-D, the first and the last row, the limits
    CHECK(verdict(4, rows, 100, 2, pos, 3, 0.5, 1) == 0);
    CHECK(verdict(4, rows, 100, 3, pos, 2, 0.5, 16) == 0);
    CHECK(verdict(4, rows, 100, 0, nullptr, 3, 0.5, 1) == 0);
    CHECK(verdict(0, nullptr, 100, 2, pos, 3, 1e-300, 1) == 0);
    CHECK(verdict(1, rows, 8, 1, pos, 3, 1e300, 1) == 0);
    std::vector<int64_t> all(kMaxTracers);
    for (int k = 0; k < kMaxTracers; ++k) all[(size_t)k] = kMaxTracers - 1 - k;
    std::vector<double> many((size_t)3 * kMaxTracers, 0.25);
    CHECK(verdict(kMaxTracers, all.data(), kMaxTracers, kMaxTracers, many.data(), 3, 0.5, 1) == 0);
    // both counts zero disables: nothing else is looked at
    CHECK(verdict(0, nullptr, 100, 0, nullptr, 3, kNaN, 0) == 0);
    CHECK(verdict(0, rows, 0, 0, pos, 2, -1.0, -5) == 0);
    // counts out of range
    CHECK(verdict(-1, rows, 100, 0, nullptr, 3, 0.5, 1) == 1);
    CHECK(verdict(0, nullptr, 100, -1, pos, 3, 0.5, 1) == 1);
    all.push_back(kMaxTracers);
    CHECK(verdict(kMaxTracers + 1, all.data(), 1 << 20, 0, nullptr, 3, 0.5, 1) == 1);
    many.resize((size_t)3 * (kMaxTracers + 1), 0.25);
    CHECK(verdict(0, nullptr, 100, kMaxTracers + 1, many.data(), 3, 0.5, 1) == 1);
    // null tables
    CHECK(verdict(4, nullptr, 100, 2, pos, 3, 0.5, 1) == 1);
    CHECK(verdict(4, rows, 100, 2, nullptr, 3, 0.5, 1) == 1);
    // capacity_steps
    CHECK(verdict(4, rows, 100, 2, pos, 3, 0.5, 0) == 1);
    CHECK(verdict(0, nullptr, 100, 2, pos, 3, 0.5, -3) == 1);
    // min_weight: finite and positive
    for (double w : {0.0, -0.0, -0.5, kInf, -kInf, kNaN}) CHECK(verdict(4, rows, 100, 2, pos, 3, w, 1) == 1);
    // rows: outside [0, n), named twice — wherever in the table
    CHECK(verdict(4, rows, 99, 0, nullptr, 3, 0.5, 1) == 1);                 // 99 is not a row of 99
    const int64_t negative[3] = {5, -1, 2}, twice[4] = {5, 9, 2, 5}, adjacent[2] = {4, 4};
    CHECK(verdict(3, negative, 100, 0, nullptr, 3, 0.5, 1) == 1);
    CHECK(verdict(4, twice, 100, 0, nullptr, 3, 0.5, 1) == 1);
    CHECK(verdict(2, adjacent, 100, 0, nullptr, 3, 0.5, 1) == 1);
    CHECK(verdict(1, rows, 0, 0, nullptr, 3, 0.5, 1) == 1);                  // a handle without rows has no row 7
    const int64_t huge[1] = {int64_t(1) << 40};
    CHECK(verdict(1, huge, 1 << 20, 0, nullptr, 3, 0.5, 1) == 1);
    // coordinates: every one of n_drifters x dims is looked at, none beyond
    for (int k = 0; k < 6; ++k)
        for (double bad : {kNaN, kInf, -kInf}) {
            double q[6];
            memcpy(q, pos, sizeof(q));
            q[k] = bad;
            CHECK(verdict(0, nullptr, 100, 2, q, 3, 0.5, 1) == 1);
            CHECK(verdict(0, nullptr, 100, 3, q, 2, 0.5, 1) == 1);
            CHECK(verdict(0, nullptr, 100, 2, q, 2, 0.5, 1) == (k < 4 ? 1 : 0));
        }
}

static void test_deliver() {
    // two tracked particles and three drifters, two steps: the payload of a step is split where the kinds meet
    const int np = 2, nd = 3, per = kTrParticleValues * np + kTrDrifterValues * nd;
    std::vector<double> step0((size_t)per), step1((size_t)per);
    for (int k = 0; k < per; ++k) { step0[(size_t)k] = 100.0 + k; step1[(size_t)k] = 200.0 + k; }
    std::vector<double> particles((size_t)2 * kTrParticleValues * np, -1.0), drifters((size_t)2 * kTrDrifterValues * nd, -1.0);
    deliver_tracers(np, nd, 0, step0.data(), particles.data(), drifters.data());
    deliver_tracers(np, nd, 1, step1.data(), particles.data(), drifters.data());
    for (int k = 0; k < kTrParticleValues * np; ++k) CHECK(particles[(size_t)k] == 100.0 + k && particles[(size_t)(kTrParticleValues * np + k)] == 200.0 + k);
    for (int k = 0; k < kTrDrifterValues * nd; ++k)
        CHECK(drifters[(size_t)k] == 100.0 + kTrParticleValues * np + k && drifters[(size_t)(kTrDrifterValues * nd + k)] == 200.0 + kTrParticleValues * np + k);
    // null outputs and absent kinds: nothing is touched, nothing is read beyond the payload
    deliver_tracers(np, nd, 0, step0.data(), nullptr, nullptr);
    std::vector<double> only_d((size_t)kTrDrifterValues * nd, -1.0), only_p((size_t)kTrParticleValues * np, -1.0);
    deliver_tracers(0, nd, 0, step0.data(), nullptr, only_d.data());
    CHECK(only_d[0] == 100.0 && only_d.back() == 100.0 + kTrDrifterValues * nd - 1);
    deliver_tracers(np, 0, 0, step0.data(), only_p.data(), nullptr);
    CHECK(only_p[0] == 100.0 && only_p.back() == 100.0 + kTrParticleValues * np - 1);
    // through a series: the record of the device-side log { iteration, time, dt, payload } is decoded and handed out in order
    StepSeries s;
    s.reset(per, 1);
    std::vector<double> rec((size_t)(kStepHeader + per));
    for (int it = 1; it <= 3; ++it) {
        const int64_t iteration = it;
        memcpy(&rec[0], &iteration, 8); rec[1] = 0.5 * it; rec[2] = 0.5;
        for (int k = 0; k < per; ++k) rec[(size_t)(kStepHeader + k)] = 1000.0 * it + k;
        s.push(StepSeries::decode(rec.data(), kStepHeader, per));
    }
    int64_t iteration = 0, n = 0, dropped = 0;
    double time = 0, dt = 0;
    s.read("sphmi_tracers_read", 4, &iteration, &time, &dt, &n, &dropped,
           [&](int64_t k, const double* v) { deliver_tracers(np, nd, k, v, particles.data(), drifters.data()); });
    CHECK(n == 1 && dropped == 2 && iteration == 3 && time == 1.5 && dt == 0.5);       // capacity 1: the newest stays, two are counted
    CHECK(particles[0] == 3000.0 && drifters[0] == 3000.0 + kTrParticleValues * np);
}

int main() {
    test_table();
    test_deliver();
    printf("%d checks\nok\n", g_checks);
    return 0;
}
