// The host side of the per-step moment sums (sphexample_amd/csrc/sphmi_series.h: check_probe_table under the name of either entry
// point, deliver_probe_moments over kPmOutputs) on hand-built tables and records: built with the host compiler and the address /
// undefined-behaviour sanitizers by tests/test_probe_moments_host.py, run as a child process.  Exit code 0 and "ok" on the last
// line: every check held.
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

// 0: accepted; 1: refused with SPHMI_ERR_ARGUMENT and the prefix of `fn`; 2: refused some other way
static int verdict(const char* fn, int32_t n, const double* pos, int dims, int64_t cap) {
    try {
        if (fn) check_probe_table(n, pos, dims, cap, fn); else check_probe_table(n, pos, dims, cap);
    } catch (const EngineError& e) {
        const std::string prefix = std::string(fn ? fn : "sphmi_probes_enable") + ": ";
        return e.status == SPHMI_ERR_ARGUMENT && std::string(e.what()).rfind(prefix, 0) == 0 ? 1 : 2;
    }
    return 0;
}

static void test_table() {
    CHECK(kMaxProbes == SPHMI_MAX_PROBES && kPrValues == 7 && kPmValues == 31);
    const double pos[6] = {0.1, 0.2, 0.3, -4.0, 5.0, 1e300};
    std::vector<double> many((size_t)3 * (kMaxProbes + 1), 0.25);
    // one check serves both entry points: the same verdicts, each under its own name
    for (const char* fn : {(const char*)nullptr, "sphmi_probe_moments_enable"}) {
        CHECK(verdict(fn, 2, pos, 3, 1) == 0 && verdict(fn, 3, pos, 2, 16) == 0);
        CHECK(verdict(fn, kMaxProbes, many.data(), 3, 1) == 0);
        CHECK(verdict(fn, 0, nullptr, 3, 0) == 0 && verdict(fn, 0, pos, 2, -5) == 0);          // n_probes = 0 disables: nothing else is looked at
        CHECK(verdict(fn, -1, pos, 3, 1) == 1 && verdict(fn, kMaxProbes + 1, many.data(), 3, 1) == 1);
        CHECK(verdict(fn, 2, nullptr, 3, 1) == 1);
        CHECK(verdict(fn, 2, pos, 3, 0) == 1 && verdict(fn, 2, pos, 3, -3) == 1);
        for (int k = 0; k < 6; ++k)
            for (double bad : {kNaN, kInf, -kInf}) {
                double q[6];
                memcpy(q, pos, sizeof(q));
                q[k] = bad;
                CHECK(verdict(fn, 2, q, 3, 1) == 1 && verdict(fn, 3, q, 2, 1) == 1);
                CHECK(verdict(fn, 2, q, 2, 1) == (k < 4 ? 1 : 0));                              // every one of n_probes x dims, none beyond
            }
    }
}

// slot s of probe p at step `step` of the hand-built record
static double value(int step, int p, int s) { return 10000.0 * (step + 1) + 100.0 * p + s; }

static void test_deliver() {
    // the widths of the caller's arrays, in the order of the C prototype behind weight_out and count_out
    const int width[8] = {1, 1, 3, 3, 6, 3, 3, 9};
    const int n_entries = (int)(sizeof(kPmOutputs) / sizeof(kPmOutputs[0]));
    CHECK(n_entries == 8);
    for (int i = 0; i < n_entries; ++i) CHECK(kPmOutputs[i].width == width[i]);
    const int np = 3, steps = 2;
    std::vector<std::vector<double>> rec((size_t)steps, std::vector<double>((size_t)kPmValues * np));
    for (int k = 0; k < steps; ++k)
        for (int p = 0; p < np; ++p)
            for (int s = 0; s < kPmValues; ++s) rec[(size_t)k][(size_t)(kPmValues * p + s)] = s == 6 ? (double)(40 + p + 10 * k) : value(k, p, s);
    std::vector<double> weight((size_t)steps * np, -1.0);
    std::vector<int64_t> count((size_t)steps * np, -1);
    std::vector<std::vector<double>> arr;
    for (int i = 0; i < n_entries; ++i) arr.emplace_back((size_t)steps * np * width[i], -1.0);
    double* const outs[8] = {arr[0].data(), arr[1].data(), arr[2].data(), arr[3].data(), arr[4].data(), arr[5].data(), arr[6].data(), arr[7].data()};
    {
        const RawOutputs out(kPmOutputs, weight.data(), count.data(), outs);
        CHECK(out.values == kPmValues && out.entries == 8);
        for (int k = 0; k < steps; ++k) deliver_probe_moments(np, k, rec[(size_t)k].data(), out);
    }
    // by hand: where every slot of the device's record lands
    const int first[8] = {1, 2, 3, 7, 10, 16, 19, 22};
    for (int k = 0; k < steps; ++k)
        for (int p = 0; p < np; ++p) {
            const size_t at = (size_t)k * np + p;
            CHECK(weight[at] == value(k, p, 0) && count[at] == 40 + p + 10 * k);
            for (int i = 0; i < n_entries; ++i)
                for (int c = 0; c < width[i]; ++c) CHECK(arr[(size_t)i][(size_t)width[i] * at + c] == value(k, p, first[i] + c));
        }
    // moment2 is six values per probe (xx, xy, xz, yy, yz, zz: slots 10 … 15), moment_velocity nine, entry 3 a + b at slot 22 + 3 a + b
    CHECK(arr[4][6 * (1 * np + 2) + 5] == value(1, 2, 15) && arr[7][9 * (0 * np + 1) + 3 * 2 + 1] == value(0, 1, 22 + 7));
    // null outputs: only what is asked for is written, nothing is read beyond the record
    std::vector<double> only((size_t)np * 6, -1.0);
    double* const some[8] = {nullptr, nullptr, nullptr, nullptr, only.data(), nullptr, nullptr, nullptr};
    {
        const RawOutputs out(kPmOutputs, nullptr, nullptr, some);
        deliver_probe_moments(np, 0, rec[0].data(), out);
    }
    CHECK(only[0] == value(0, 0, 10) && only.back() == value(0, np - 1, 15));
    double* const none[8] = {};
    {
        const RawOutputs out(kPmOutputs, nullptr, nullptr, none);
        deliver_probe_moments(np, 0, rec[0].data(), out);
        deliver_probe_moments(0, 0, nullptr, out);
    }
    // through a series: the record of the device-side log { iteration, time, dt, payload } is decoded and handed out in order
    StepSeries s;
    s.reset(kPmValues * np, 2);
    std::vector<double> log((size_t)(kStepHeader + kPmValues * np));
    for (int it = 1; it <= 3; ++it) {
        const int64_t iteration = it;
        memcpy(&log[0], &iteration, 8); log[1] = 0.5 * it; log[2] = 0.5;
        for (int p = 0; p < np; ++p)
            for (int q = 0; q < kPmValues; ++q) log[(size_t)(kStepHeader + kPmValues * p + q)] = value(it, p, q);
        s.push(StepSeries::decode(log.data(), kStepHeader, kPmValues * np));
    }
    int64_t iteration[2] = {0, 0}, n = 0, dropped = 0;
    double time[2] = {0, 0}, dt[2] = {0, 0};
    {
        const RawOutputs out(kPmOutputs, weight.data(), count.data(), outs);
        s.read("sphmi_probe_moments_read", 0, nullptr, nullptr, nullptr, &n, &dropped, [&](int64_t, const double*) { CHECK(false); });
        CHECK(n == 2 && dropped == 1);                                              // capacity = 0 is a question
        s.read("sphmi_probe_moments_read", 2, iteration, time, dt, &n, &dropped, [&](int64_t k, const double* v) { deliver_probe_moments(np, k, v, out); });
    }
    CHECK(n == 2 && dropped == 1 && iteration[0] == 2 && iteration[1] == 3 && time[1] == 1.5 && dt[0] == 0.5);
    CHECK(weight[0] == value(2, 0, 0) && weight[(size_t)np] == value(3, 0, 0) && arr[7][(size_t)9 * (np + 2) + 8] == value(3, 2, 30));
}

int main() {
    test_table();
    test_deliver();
    printf("%d checks\nok\n", g_checks);
    return 0;
}
