// The plain C++ part of sphexample_amd/csrc/sphmi_select.h — SelSpec, SelRow, sel_speed2 and sel_keep, the functions k_sel_flag runs on
// the device — compiled for the host (with the sanitizers where their runtime links) and run on the cases tests/test_select_host.py
// writes to stdin.  Every number travels as a C99 hex float or a decimal integer:
//
//     case <type_mask> <dims> <n_boxes> <n_markers> <id_stride> <id_phase> <field> <field_lo> <field_hi> <has_mask> <n_rows>
//     box <lo0> <lo1> <lo2> <hi0> <hi1> <hi2>                                     n_boxes lines
//     marker <m>                                                                  n_markers lines
//     row <type> <x> <y> <z> <vx> <vy> <vz> <density> <pressure> <id> <group> <mask>      n_rows lines
//
// and every case answers one line, "kept <count> <row> <row> …", ascending; "ok" ends the output.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "sphmi_select.h"

using namespace sphmi;

static bool word(std::string& w) {
    char buf[128];
    if (scanf("%127s", buf) != 1) return false;
    w = buf;
    return true;
}
static double number() {
    std::string w;
    if (!word(w)) { fprintf(stderr, "input ends inside a case\n"); exit(2); }
    char* end = nullptr;
    const double v = strtod(w.c_str(), &end);
    if (end == w.c_str() || *end) { fprintf(stderr, "not a number: %s\n", w.c_str()); exit(2); }
    return v;
}
static long long integer() {
    std::string w;
    if (!word(w)) { fprintf(stderr, "input ends inside a case\n"); exit(2); }
    char* end = nullptr;
    const long long v = strtoll(w.c_str(), &end, 10);
    if (end == w.c_str() || *end) { fprintf(stderr, "not an integer: %s\n", w.c_str()); exit(2); }
    return v;
}
static unsigned long long natural() {
    std::string w;
    if (!word(w)) { fprintf(stderr, "input ends inside a case\n"); exit(2); }
    char* end = nullptr;
    const unsigned long long v = strtoull(w.c_str(), &end, 10);
    if (end == w.c_str() || *end) { fprintf(stderr, "not an integer: %s\n", w.c_str()); exit(2); }
    return v;
}
static void expect(const char* tag) {
    std::string w;
    if (!word(w) || w != tag) { fprintf(stderr, "expected `%s`, read `%s`\n", tag, w.c_str()); exit(2); }
}

int main() {
    std::string w;
    int cases = 0;
    while (word(w)) {
        if (w != "case") { fprintf(stderr, "expected `case`, read `%s`\n", w.c_str()); return 2; }
        SelSpec s;
        memset(&s, 0, sizeof(s));
        s.type_mask = (uint32_t)integer(); s.dims = (int32_t)integer(); s.n_boxes = (int32_t)integer(); s.n_markers = (int32_t)integer();
        s.id_stride = integer(); s.id_phase = integer(); s.field = (int32_t)integer();
        s.field_lo = number(); s.field_hi = number(); s.has_mask = (int32_t)integer();
        const long long n = integer();
        if (s.n_boxes < 0 || s.n_boxes > kSelMaxBoxes || s.n_markers < 0 || s.n_markers > kSelMaxMarkers || n < 0 || (s.dims != 2 && s.dims != 3)) {
            fprintf(stderr, "case %d: counts out of range\n", cases);
            return 2;
        }
        for (int b = 0; b < s.n_boxes; ++b) {
            expect("box");
            for (int d = 0; d < 3; ++d) s.lo[b][d] = number();
            for (int d = 0; d < 3; ++d) s.hi[b][d] = number();
        }
        for (int k = 0; k < s.n_markers; ++k) { expect("marker"); s.markers[k] = natural(); }
        std::vector<long long> kept;
        for (long long i = 0; i < n; ++i) {
            expect("row");
            SelRow r;
            memset(&r, 0, sizeof(r));
            r.type = (int32_t)integer();
            for (int d = 0; d < 3; ++d) r.x[d] = number();
            double v[3];
            for (int d = 0; d < 3; ++d) v[d] = number();
            const double density = number(), pressure = number();
            r.id = integer(); r.group = natural(); r.mask = (uint8_t)integer();
            // the value of the field clause, as k_sel_flag forms it
            if (s.field == kSelFieldDensity) r.value = density;
            else if (s.field == kSelFieldPressure) r.value = pressure;
            else if (s.field == kSelFieldSpeed2) r.value = sel_speed2(v[0], v[1], s.dims == 3 ? v[2] : 0.0);
            if (sel_keep(s, r)) kept.push_back(i);
        }
        printf("kept %zu", kept.size());
        for (long long i : kept) printf(" %lld", i);
        printf("\n");
        cases += 1;
    }
    printf("ok\n");
    return 0;
}
