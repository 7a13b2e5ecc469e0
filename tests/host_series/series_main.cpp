// The observers' host-side series (sphexample_amd/csrc/sphmi_series.h) on its own: built with the host compiler and the
// address / undefined-behaviour sanitizers by tests/test_step_series_host.py, run as a child process.  Exit code 0 and "ok"
// on the last line: every check held.
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

static const char* kFn = "sphmi_group_forces_read";

// a device-side record of `values` payload doubles: { iteration (int64 bits), time, Δt, payload }, payload[c] = 100·it + c + ¼
static std::vector<double> record(int64_t it, int values) {
    std::vector<double> r((size_t)kStepHeader + values);
    memcpy(&r[0], &it, 8);
    r[1] = 0.5 * (double)it; r[2] = 0.125 + (double)it;
    for (int c = 0; c < values; ++c) r[(size_t)kStepHeader + c] = 100.0 * (double)it + c + 0.25;
    return r;
}
static void push(StepSeries& s, int64_t it) { s.push(StepSeries::decode(record(it, s.values).data(), kStepHeader, s.values)); }

struct Got {
    std::vector<int64_t> it; std::vector<double> t, dt, v;
    int64_t n = -7, dropped = -7;
};
// a read of at most `cap` samples into arrays of exactly that size (the sanitizer sees a write past them)
static Got read(StepSeries& s, int64_t cap) {
    Got g;
    g.it.assign((size_t)cap, -1); g.t.assign((size_t)cap, -1.0); g.dt.assign((size_t)cap, -1.0); g.v.assign((size_t)cap * s.values, -1.0);
    s.read(kFn, cap, g.it.data(), g.t.data(), g.dt.data(), &g.n, &g.dropped, [&](int64_t k, const double* v) { deliver_forces(s.values / 3, k, v, g.v.data()); });
    return g;
}
static void check_sample(const Got& g, int64_t k, int64_t it, int values) {
    const std::vector<double> r = record(it, values);
    CHECK(g.it[(size_t)k] == it);
    CHECK(g.t[(size_t)k] == r[1] && g.dt[(size_t)k] == r[2]);
    CHECK(memcmp(&g.v[(size_t)k * values], &r[kStepHeader], (size_t)values * 8) == 0);
}

// capacity 1 and 3, 0 / 1 / capacity / capacity + 2 pushes: the newest `capacity` samples wait, the others count as dropped
static void test_ring() {
    const int values = 6;
    for (int64_t capacity : {1, 3}) {
        for (int64_t pushes : {(int64_t)0, (int64_t)1, capacity, capacity + 2}) {
            StepSeries s;
            s.reset(values, capacity);
            for (int64_t it = 1; it <= pushes; ++it) push(s, it);
            const int64_t kept = std::min(pushes, capacity), lost = pushes - kept;
            // the question: cap == 0 delivers nothing, clears nothing, leaves `dropped` standing — asked twice
            for (int rep = 0; rep < 2; ++rep) {
                int64_t n = -1, d = -1;
                s.read(kFn, 0, nullptr, nullptr, nullptr, &n, &d, [&](int64_t, const double*) { CHECK(false); });
                CHECK(n == kept && d == lost);
                CHECK((int64_t)s.q.size() == kept && s.dropped == lost);
            }
            Got g = read(s, capacity + 1);
            CHECK(g.n == kept && g.dropped == lost);
            for (int64_t k = 0; k < kept; ++k) check_sample(g, k, pushes - kept + 1 + k, values);
            for (size_t k = (size_t)kept; k < g.it.size(); ++k) CHECK(g.it[k] == -1 && g.t[k] == -1.0);       // nothing behind the delivered ones
            // the delivering read reset `dropped`; a second read finds nothing
            g = read(s, capacity + 1);
            CHECK(g.n == 0 && g.dropped == 0 && s.q.empty());
        }
    }
}

// cap smaller than the queue, then the rest; `dropped` is handed over by the first delivering read only — also one that delivers 0 samples
static void test_partial_read_and_dropped() {
    StepSeries s;
    s.reset(3, 3);
    for (int64_t it = 1; it <= 5; ++it) push(s, it);           // 3, 4, 5 wait; 2 dropped
    Got g = read(s, 2);
    CHECK(g.n == 2 && g.dropped == 2);
    check_sample(g, 0, 3, 3); check_sample(g, 1, 4, 3);
    int64_t n = -1, d = -1;
    s.read(kFn, 0, nullptr, nullptr, nullptr, &n, &d, [&](int64_t, const double*) { CHECK(false); });
    CHECK(n == 1 && d == 0);
    push(s, 6);
    g = read(s, 2);
    CHECK(g.n == 2 && g.dropped == 0);
    check_sample(g, 0, 5, 3); check_sample(g, 1, 6, 3);
    // an empty series with a drop count: capacity 1, two pushes, one read takes the sample and the count
    s.reset(3, 1);
    push(s, 1); push(s, 2);
    g = read(s, 1);
    CHECK(g.n == 1 && g.dropped == 1);
    g = read(s, 1);
    CHECK(g.n == 0 && g.dropped == 0);
    // reset clears the queue and the count
    push(s, 3); push(s, 4);
    s.reset(3, 2);
    CHECK(s.q.empty() && s.dropped == 0 && s.capacity == 2);
}

static void test_argument_errors() {
    StepSeries s;
    s.reset(3, 2);
    push(s, 1);
    auto nothing = [&](int64_t, const double*) { CHECK(false); };
    int64_t n = -1;
    for (const char* fn : {"sphmi_group_forces_read", "sphmi_probes_read"}) {
        try { s.read(fn, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nothing); CHECK(false); }
        catch (const EngineError& e) { CHECK(e.status == SPHMI_ERR_ARGUMENT && std::string(e.what()) == std::string(fn) + ": null n_out"); }
        try { s.read(fn, -1, nullptr, nullptr, nullptr, &n, nullptr, nothing); CHECK(false); }
        catch (const EngineError& e) { CHECK(e.status == SPHMI_ERR_ARGUMENT && std::string(e.what()) == std::string(fn) + ": negative capacity"); }
    }
    CHECK(n == -1 && s.q.size() == 1);                         // a refused read touches nothing
    // every optional output null: the sample still leaves the series
    int delivered = 0;
    s.read(kFn, 4, nullptr, nullptr, nullptr, &n, nullptr, [&](int64_t k, const double* v) {
        delivered += 1;
        CHECK(k == 0 && v[0] == 100.25);
        deliver_forces(1, k, v, nullptr);
        deliver_probe_means(0, k, v, nullptr, nullptr, nullptr, nullptr, nullptr);
    });
    CHECK(n == 1 && delivered == 1 && s.q.empty());
}

static void test_add() {
    const int values = 6;
    StepSeries::Sample a = StepSeries::decode(record(7, values).data(), kStepHeader, values);
    const StepSeries::Sample b = StepSeries::decode(record(7, values).data(), kStepHeader, values);
    StepSeries::Sample c = StepSeries::decode(record(8, values).data(), kStepHeader, values);
    c.v[2] = 0.1;
    const StepSeries::Sample a0 = a;
    StepSeries::add(a, b, "probes");
    for (int k = 0; k < values; ++k) CHECK(a.v[(size_t)k] == a0.v[(size_t)k] + b.v[(size_t)k]);
    CHECK(a.iteration == 7 && a.time == a0.time && a.dt == a0.dt);
    for (const char* what : {"group forces", "probes"}) {
        const StepSeries::Sample before = a;
        try { StepSeries::add(a, c, what); CHECK(false); }
        catch (const EngineError& e) {
            CHECK(e.status == SPHMI_ERR_STATE && std::string(e.what()) == std::string(what) + ": the slabs' records of a step do not belong together");
        }
        CHECK(a.v == before.v);                                // nothing was added
    }
}

// the group-force payload travels record → sample → caller bit for bit: NaN payloads, signed zeros, subnormals, infinities
static void test_forces_bit_for_bit() {
    const int n_groups = 2, values = 3 * n_groups;
    const uint64_t bits[values] = {0x7ff8000000000abcull, 0x8000000000000000ull, 0x0000000000000001ull, 0xfff0000000000000ull, 0x3ff0000000000001ull, 0x7ff4000000000001ull};
    std::vector<double> rec = record(std::numeric_limits<int64_t>::min() + 5, values);
    memcpy(&rec[kStepHeader], bits, sizeof bits);
    StepSeries s;
    s.reset(values, 2);
    s.push(StepSeries::decode(rec.data(), kStepHeader, values));
    push(s, 2);
    Got g = read(s, 2);
    CHECK(g.n == 2 && g.it[0] == std::numeric_limits<int64_t>::min() + 5);
    CHECK(memcmp(g.v.data(), bits, sizeof bits) == 0);
    check_sample(g, 1, 2, values);
}

static void test_probe_means() {
    const int n_probes = 3;
    // { S, SP, Sρ, Sv[3], n }: a probe with rows, one with n == 0 (sums that must not show), one with rows and S == 0
    const double sums[n_probes * kPrValues] = {
        0.75, 1.5, 750.0, 0.3, -0.6, 0.9, 4.0,
        0.5, 9.0, 9.0, 9.0, 9.0, 9.0, 0.0,
        0.0, 9.0, 9.0, 9.0, 9.0, 9.0, 2.0};
    std::vector<double> rec = record(11, n_probes * kPrValues);
    memcpy(&rec[kStepHeader], sums, sizeof sums);
    StepSeries s;
    s.reset(n_probes * kPrValues, 4);
    s.push(StepSeries::decode(rec.data(), kStepHeader, s.values));
    s.push(StepSeries::decode(rec.data(), kStepHeader, s.values));
    const int64_t cap = 2;
    std::vector<double> w((size_t)cap * n_probes, -1.0), P(w), rho(w), vel((size_t)cap * n_probes * 3, -1.0);
    std::vector<int64_t> cnt((size_t)cap * n_probes, -1);
    int64_t n = 0;
    s.read("sphmi_probes_read", cap, nullptr, nullptr, nullptr, &n, nullptr, [&](int64_t k, const double* v) {
        deliver_probe_means(n_probes, k, v, w.data(), cnt.data(), P.data(), rho.data(), vel.data());
    });
    CHECK(n == 2);
    for (size_t k = 0; k < 2; ++k) {
        const size_t at = k * n_probes;
        CHECK(w[at] == 0.75 && cnt[at] == 4 && P[at] == 1.5 / 0.75 && rho[at] == 750.0 / 0.75);
        CHECK(vel[3 * at] == 0.3 / 0.75 && vel[3 * at + 1] == -0.6 / 0.75 && vel[3 * at + 2] == 0.9 / 0.75);
        CHECK(w[at + 1] == 0.5 && cnt[at + 1] == 0 && w[at + 2] == 0.0 && cnt[at + 2] == 2);         // weight and count: as summed
        for (size_t p = 1; p < 3; ++p) {
            CHECK(P[at + p] == 0.0 && rho[at + p] == 0.0);
            for (int d = 0; d < 3; ++d) CHECK(vel[3 * (at + p) + d] == 0.0);
        }
    }
    // the lattice forms its means with the same function
    CHECK(kernel_mean(1.5, 0.75, true) == 1.5 / 0.75 && kernel_mean(1.5, 0.75, false) == 0.0 && kernel_mean(9.0, 0.0, false) == 0.0);
    double gw[2] = {-1, -1}, gp[2] = {-1, -1}, gv[6]; int64_t gc[2] = {-1, -1};
    GridSums G(2, gw, gc, gp, nullptr, gv);
    CHECK(G.want[0] && G.want[1] && !G.want[2] && G.want[3] && G.want[6] && G.dst(0) == gw);
    const double node[2][kFgValues] = {{0.75, 1.5, 0, 0.3, -0.6, 0.9, 4.0}, {0.5, 9, 9, 9, 9, 9, 0.0}};
    for (int f = 0; f < kFgValues; ++f) if (G.want[f]) for (int k = 0; k < 2; ++k) G.dst(f)[k] = node[k][f];
    G.deliver(gc, gp, nullptr, gv);
    CHECK(gc[0] == 4 && gc[1] == 0 && gp[0] == P[0] && gp[1] == 0.0);
    for (int d = 0; d < 3; ++d) CHECK(gv[d] == vel[(size_t)d] && gv[3 + d] == 0.0);
}

// The raw outputs of the gradients and the moments (RawOutputs over its table, through GridSums): for EVERY subset of the outputs
// of a 3-point call, exactly the slots of the requested outputs are wanted, slot f filled with 100·f + k arrives as entry (k, c) =
// 100·(first + c) + k of the output that holds it, count is the integer of slot 6, weight is slot 0 written in place, and a NULL
// output receives nothing — wanted() and deliver() read one table, and this is the check that they agree.  The arrays have exactly
// the size a caller gives them (the sanitizer sees a write past them).
template <int N> static void test_raw_outputs(const OutputSlots (&table)[N], int values) {
    const int64_t n = 3;
    CHECK(values <= kSampleValuesMax && N <= kRawOutputsMax);
    for (unsigned subset = 0; subset < (1u << (N + 2)); ++subset) {           // bit 0: weight, bit 1: count, bit 2 + i: output i
        std::vector<double> weight((size_t)n, -1.0);
        std::vector<int64_t> count((size_t)n, -1);
        std::vector<double> arrays[N];
        double* ptr[N];
        bool expect[kSampleValuesMax] = {};
        expect[0] = subset & 1u; expect[6] = (subset >> 1) & 1u;
        for (int i = 0; i < N; ++i) {
            const bool on = (subset >> (2 + i)) & 1u;
            arrays[i].assign((size_t)n * table[i].width, -1.0);
            ptr[i] = on ? arrays[i].data() : nullptr;
            for (int c = 0; c < table[i].width; ++c) expect[table[i].first + c] = on;
        }
        const RawOutputs out(table, (subset & 1u) ? weight.data() : nullptr, (subset & 2u) ? count.data() : nullptr, ptr);
        CHECK(out.values == values && out.entries == N);
        GridSums G(n, out);
        CHECK(G.nodes == n && G.values == values);
        for (int f = 0; f < kSampleValuesMax; ++f) CHECK(G.want[f] == expect[f]);
        CHECK((subset & 1u) ? G.dst(0) == weight.data() : true);
        for (int f = 0; f < values; ++f) {
            if (!G.want[f]) { CHECK(f == 0 || G.s[f].empty()); continue; }   // no host allocation for a slot nobody asked for
            for (int64_t k = 0; k < n; ++k) G.dst(f)[k] = 100.0 * f + (double)k;
        }
        int visited = 0;
        G.for_wanted([&](int f, double* dst) { CHECK(expect[f] && dst == G.dst(f)); visited += 1; });
        int expected = 0;
        for (int f = 0; f < values; ++f) expected += expect[f];
        CHECK(visited == expected);
        out.deliver(G);
        for (int64_t k = 0; k < n; ++k) {
            CHECK(weight[(size_t)k] == ((subset & 1u) ? (double)k : -1.0));
            CHECK(count[(size_t)k] == ((subset & 2u) ? 600 + k : -1));
            for (int i = 0; i < N; ++i)
                for (int c = 0; c < table[i].width; ++c)
                    CHECK(arrays[i][(size_t)(table[i].width * k + c)] == (ptr[i] ? 100.0 * (table[i].first + c) + (double)k : -1.0));
        }
    }
}

int main() {
    test_raw_outputs(kPgOutputs, kPgValues);                   // 2⁹ subsets
    test_raw_outputs(kPmOutputs, kPmValues);                   // 2¹⁰ subsets
    test_ring();
    test_partial_read_and_dropped();
    test_argument_errors();
    test_add();
    test_forces_bit_for_bit();
    test_probe_means();
    printf("%d checks\nok\n", g_checks);
    return 0;
}
