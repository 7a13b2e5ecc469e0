// The host side of the per-particle envelopes (sphexample_amd/csrc/sphmi_series.h: check_envelope_mask, deliver_envelope_window,
// deliver_envelope_speed) on hand-made masks, headers and arrays: built with the host compiler and the address /
// undefined-behaviour sanitizers by tests/test_envelopes_host.py, run as a child process.  Exit code 0 and "ok" on the last line:
// every check held.
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

static bool refused(uint32_t mask) {
    try { check_envelope_mask(mask); }
    catch (const EngineError& e) { return e.status == SPHMI_ERR_ARGUMENT && std::string(e.what()).rfind("sphmi_envelopes_enable: ", 0) == 0; }
    return false;
}

static void test_mask() {
    CHECK(kEnValues == 8 && kEnHeader == 4);
    // every subset of the bits 1 (Fluid), 2 (Fixed), 3 (Moving) is a selection, the empty one disables
    for (uint32_t m = 0; m < 16; m += 2) CHECK(!refused(m));
    // bit 0 is no Type, nor is any bit above 3 - alone or next to legal ones
    CHECK(refused(1u)); CHECK(refused(1u << 4)); CHECK(refused((1u << 1) | 1u)); CHECK(refused(0xEu | (1u << 31)));
    for (int b = 4; b < 32; ++b) CHECK(refused((1u << b) | (1u << 1)));
}

static void test_window() {
    // the header as the device keeps it: the step count is an int64 carried in the bits of a double
    double header[kEnHeader];
    const int64_t steps = (int64_t(1) << 40) + 7;
    memcpy(&header[0], &steps, 8);
    header[1] = 0.125; header[2] = 0.625; header[3] = 0.5;
    int64_t got = -1;
    std::vector<double> window(3, kNaN);               // exactly three doubles: the sanitizer sees a write past them
    deliver_envelope_window(header, &got, window.data());
    CHECK(got == steps && window[0] == 0.125 && window[1] == 0.625 && window[2] == 0.5);
    // either output may be absent
    got = -1;
    deliver_envelope_window(header, &got, nullptr);
    CHECK(got == steps);
    window.assign(3, kNaN);
    deliver_envelope_window(header, nullptr, window.data());
    CHECK(window[2] == 0.5);
    deliver_envelope_window(header, nullptr, nullptr);
    // a window of no steps: the bits of +0.0 are the count 0
    const double fresh[kEnHeader] = {0.0, 2.0, 2.0, 0.0};
    deliver_envelope_window(fresh, &got, window.data());
    CHECK(got == 0 && window[0] == 2.0 && window[1] == 2.0 && window[2] == 0.0);
}

static void test_speed() {
    // max |v|^2 -> the largest speed, in place, correctly rounded; the start record 0 stays 0, NaN stays NaN
    std::vector<double> s = {0.0, 4.0, 2.0, 1e-300, kInf, kNaN, 0.25};
    const std::vector<double> in = s;
    deliver_envelope_speed((int64_t)s.size(), s.data());
    CHECK(s[0] == 0.0 && !std::signbit(s[0]) && s[1] == 2.0 && s[2] == std::sqrt(2.0) && s[3] == std::sqrt(1e-300) && s[4] == kInf && std::isnan(s[5]) && s[6] == 0.5);
    // a null array is skipped, no row is no work
    deliver_envelope_speed(7, nullptr);
    std::vector<double> none;
    deliver_envelope_speed(0, none.data());
    // exactly n entries are touched
    std::vector<double> two = {9.0, 16.0, 25.0};
    deliver_envelope_speed(2, two.data());
    CHECK(two[0] == 3.0 && two[1] == 4.0 && two[2] == 25.0);
    (void)in;
}

int main() {
    test_mask();
    test_window();
    test_speed();
    printf("%d checks\nok\n", g_checks);
    return 0;
}
