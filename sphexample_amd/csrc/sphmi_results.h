// sphmi_results.h — what the host side of every device-side result is built from: a typed device allocation that only grows
// (DeviceBuf), the 64-bit exclusive scan that sizes a variable-length result (scan64), the optional per-pass device timing of a
// build (PassClock) and the none / valid / stale state of a result the handle holds between calls (HeldResult).  Host code only;
// sphmi_engine.hip includes it behind HC and HostBounce, which it uses.  A new on-demand result starts from these four.
#pragma once
#include <cstdarg>
#include <initializer_list>

#include "sphmi_neighbor_list.h"

namespace sphmi {

inline std::string text(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
inline std::string text(const char* fmt, ...) {
    char buf[320];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}

// `cap` elements of U on the device.  need() leaves at least `count` of them — never less than 8 bytes, so that no request, an
// empty one included, reaches hipMalloc with 0 bytes and `p` is a pointer a kernel may be handed — and frees before it allocates:
// the peak is one copy.  The contents do not survive growing.  Released by free() only, at the places the owner chooses: there
// is no destructor, because the engine frees in a fixed order before it destroys its stream.
template <class U> struct DeviceBuf {
    U* p = nullptr;
    size_t cap = 0;
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    // on_fail(bytes) → the text of the EngineError(SPHMI_ERR_DEVICE) thrown when the device has no such memory; nothing is held then
    template <class F> void need(size_t count, F&& on_fail) {
        if (p && count <= cap) return;
        free();
        const size_t bytes = count * sizeof(U);
        if (hipMalloc((void**)&p, std::max<size_t>(bytes, 8)) != hipSuccess) {
            (void)hipGetLastError();
            p = nullptr;
            throw EngineError(SPHMI_ERR_DEVICE, on_fail(bytes));
        }
        cap = count;
    }
    void need(size_t count) {
        need(count, [](size_t bytes) { return text("hipMalloc: no device memory for %zu bytes", bytes); });
    }
    void free() {
        (void)hipFree(p);
        p = nullptr; cap = 0;
    }
};

// The exclusive scan of counts[n] (int32) into offsets[n + 1] (int64), offsets[n] the total, which it returns: k_nl_tile_sums →
// k_nl_scan_tiles → k_nl_offsets (sphmi_neighbor_list.h) on `stream`, the total through the bounce buffer — complete on return, the
// one synchronisation of the sequence.  `tsum` grows to one word per tile of kNlScanTile counts.
template <class F>
long long scan64(const int* counts, int n, DeviceBuf<long long>& tsum, long long* offsets, HostBounce& bounce, hipStream_t stream, F&& on_fail) {
    const int ntiles = (n + kNlScanTile - 1) / kNlScanTile;
    tsum.need((size_t)ntiles, on_fail);
    hipLaunchKernelGGL(k_nl_tile_sums, dim3(ntiles), dim3(kNlScanThreads), 0, stream, counts, n, tsum.p);
    hipLaunchKernelGGL(k_nl_scan_tiles, dim3(1), dim3(1024), 0, stream, tsum.p, ntiles, offsets + n);
    hipLaunchKernelGGL(k_nl_offsets, dim3(ntiles), dim3(kNlScanThreads), 0, stream, counts, n, (const long long*)tsum.p, offsets);
    HC(hipGetLastError());
    long long total = 0;
    bounce.d2h(&total, offsets + n, 8, stream);
    return total;
}

// The device time of the passes of a build, for the cost tools: with the environment variable `env` set (read at construction, so
// at every build), mark() records an event on the stream and report() — after the stream was synchronised — writes ONE line to
// stderr, `head` and then "name x.xxx ms" for every interval between two marks.  Unset: both do nothing.  The destructor destroys
// the events, also when the build throws.
struct PassClock {
    static constexpr int kMarks = 8;
    const bool on;
    hipStream_t stream;
    hipEvent_t ev[kMarks] = {};
    int n = 0;
    PassClock(const char* env, hipStream_t s) : on(getenv(env) != nullptr), stream(s) {}
    PassClock(const PassClock&) = delete;
    PassClock& operator=(const PassClock&) = delete;
    ~PassClock() { for (int k = 0; k < n; ++k) (void)hipEventDestroy(ev[k]); }
    void mark() {
        if (!on) return;
        if (n == kMarks) throw EngineError(SPHMI_ERR_DEVICE, "PassClock: more marks than kMarks");
        HC(hipEventCreate(&ev[n]));
        n += 1;
        HC(hipEventRecord(ev[n - 1], stream));
    }
    void report(const std::string& head, std::initializer_list<const char*> names) {
        if (!on) return;
        std::string line = head;
        int k = 0;
        for (const char* name : names) {
            if (k + 1 >= n) break;
            float ms = 0;
            HC(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
            line += text("%s %s %.3f ms", k ? "," : "", name, ms);
            k += 1;
        }
        fprintf(stderr, "%s\n", line.c_str());
    }
};

// Whether a result the handle holds between calls (the neighbour list, the components, the mesh, a selection) matches the rows: a build sets it
// valid, whatever moves rows — sphmi_advance, sphmi_upload, the generator, sphmi_forces_once — turns valid into stale, a release or
// a failed build leaves none.
struct HeldResult {
    enum State { NONE = 0, VALID, STALE };
    State state = NONE;
    void stale() { if (state == VALID) state = STALE; }
    void drop() { state = NONE; }
    void set_valid() { state = VALID; }
    void require_readable(const char* fn, const char* none_text, const char* stale_text) const {
        if (state == STALE) throw EngineError(SPHMI_ERR_STATE, std::string(fn) + ": " + stale_text);
        if (state != VALID) throw EngineError(SPHMI_ERR_STATE, std::string(fn) + ": " + none_text);
    }
};

}  // namespace sphmi
