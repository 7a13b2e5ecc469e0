// sphmi_series.h — the host side the observers share (group forces, probes, budgets, flow, envelopes, maps, tracers, lattice, columns): the error type, the limits and
// record-layout constants host and device agree on, the argument checks every kind of handle reports alike, the per-step series
// and the means of the kernel sums; the slot tables of the samplers that deliver raw sums (kPgOutputs, kPmOutputs: the one statement
// of their layouts on the host) and the sums of one sampler call (GridSums).  Plain C++17, no HIP: tests/host_series/series_main.cpp
// compiles it alone.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <deque>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/sphmi.h"

namespace sphmi {

struct EngineError : std::runtime_error {
    int status;
    EngineError(int s, const std::string& m) : std::runtime_error(m), status(s) {}
};

constexpr int kMaxColumns = 16;                  // SPHMI_MAX_COLUMNS
constexpr int kMaxColumnRowBytes = 64;           // SPHMI_MAX_COLUMN_ROW_BYTES
constexpr int kMaxForceGroups = 16;              // SPHMI_MAX_FORCE_GROUPS
constexpr int kStepHeader = 3;                     // doubles in front of the payload of a record: iteration (int64 bits), time, Δt
constexpr int kMaxProbes = 1024;                 // SPHMI_MAX_PROBES
constexpr int kPrValues = 7;                     // S, SP, Sρ, Sv[3], n
constexpr int kFgValues = kPrValues;             // S, SP, Sρ, Sv[3], n
constexpr long long kMaxGridNodes = 1ll << 24;   // SPHMI_MAX_GRID_NODES
constexpr long long kMaxSamplePoints = 1ll << 24; // SPHMI_MAX_SAMPLE_POINTS
constexpr int kPgValues = kFgValues + 18;        // the sums of the cloud, then G[3], GP[3], Gρ[3], Gv[3][3] (sphmi_point_gradients.h)
constexpr int kPmValues = kFgValues + 24;        // the sums of the cloud, then M1[3], M2[6], P1[3], R1[3], V1[3][3] (sphmi_point_moments.h)
constexpr int kSampleValuesMax = kPmValues;      // the most sums per node any sampler delivers through GridSums
constexpr int kBgValues = 22;                    // the raw budgets of the fluid (sphmi_budgets.h): thirteen sums, nine extremes

// How two values of slot `slot` of a budget record combine: 0 sum (slots 0 … 12), 1 min, 2 max (13 max |v|², 14 / 15 min / max ρ,
// 16 … 18 / 19 … 21 min / max x per axis).  The kernels and the host side of a multi-device handle use the same rule.
constexpr int bg_rule(int slot) { return slot < 13 ? 0 : (slot == 14 || (slot >= 16 && slot <= 18)) ? 1 : 2; }
constexpr int kMaxFlowBoxes = 16;                // SPHMI_MAX_FLOW_BOXES
constexpr int kFlValues = 7;                     // per control box (sphmi_flow.h): n_after, Σ1/ρ, Σv[3], entered, left — every slot a sum
constexpr int kEnValues = 8;                     // per row (sphmi_envelopes.h): p_max, t_p_max, p_min, impulse, square, loaded, speed2_max, t_arrival
constexpr int kEnHeader = 4;                     // the window of the envelopes: steps (int64 bits), t_begin, t_end, duration
constexpr long long kMaxMapBins = 1ll << 20;     // SPHMI_MAX_MAP_BINS
constexpr int kMpValues = 12;                    // per bin (sphmi_maps.h): top_max, t_top_max, bottom_min, t_arrival, wet, fill, flux[3], speed2_max, t_speed2_max, n_max
constexpr int kMpHeader = 4;                     // the window of the maps, as the envelopes keep it
constexpr int kMaxTracers = 1024;                // SPHMI_MAX_TRACERS: of either kind
constexpr int kTrParticleValues = 8;             // per tracked particle (sphmi_tracers.h): x[3], v[3], ρ, P
constexpr int kTrDrifterValues = 3 + kPrValues;  // per drifter: X[3], the position the sums were taken at, then S, SP, Sρ, Sv[3], n

// sphmi_attach_columns: the argument errors every kind of handle reports alike
inline void check_column_table(int32_t n_columns, const void* const* columns, const int32_t* row_bytes) {
    if (n_columns < 0 || n_columns > kMaxColumns) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_attach_columns: n_columns out of range [0, 16]");
    if (n_columns == 0) return;
    if (!columns || !row_bytes) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_attach_columns: null table");
    for (int c = 0; c < n_columns; ++c) {
        if (row_bytes[c] < 1 || row_bytes[c] > kMaxColumnRowBytes) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_attach_columns: row_bytes out of range [1, 64]");
        if (!columns[c]) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_attach_columns: null column");
    }
}

// sphmi_group_forces_enable: the argument errors every kind of handle reports alike
inline void check_group_table(int32_t n_groups, const uint64_t* markers, int64_t capacity_steps) {
    if (n_groups < 0 || n_groups > kMaxForceGroups) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_group_forces_enable: n_groups out of range [0, 16]");
    if (n_groups == 0) return;
    if (!markers) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_group_forces_enable: null table");
    if (capacity_steps < 1) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_group_forces_enable: capacity_steps must be positive");
    for (int a = 0; a < n_groups; ++a)
        for (int b = 0; b < a; ++b)
            if (markers[a] == markers[b]) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_group_forces_enable: duplicate marker");
}

// sphmi_probes_enable and sphmi_probe_moments_enable (`fn`): the argument errors every kind of handle reports alike
inline void check_probe_table(int32_t n_probes, const double* positions, int dims, int64_t capacity_steps, const char* fn = "sphmi_probes_enable") {
    const std::string name(fn);
    if (n_probes < 0 || n_probes > kMaxProbes) throw EngineError(SPHMI_ERR_ARGUMENT, name + ": n_probes out of range [0, 1024]");
    if (n_probes == 0) return;
    if (!positions) throw EngineError(SPHMI_ERR_ARGUMENT, name + ": null table");
    if (capacity_steps < 1) throw EngineError(SPHMI_ERR_ARGUMENT, name + ": capacity_steps must be positive");
    for (int64_t k = 0; k < (int64_t)n_probes * dims; ++k)
        if (!std::isfinite(positions[k])) throw EngineError(SPHMI_ERR_ARGUMENT, name + ": non-finite coordinate");
}

// sphmi_flow_enable: the argument errors every kind of handle reports alike.  A box is half-open, lo <= x < hi per axis; -inf and
// +inf are bounds like any other, NaN is none, and a box with !(lo < hi) on an axis could hold no row.
inline void check_flow_table(int32_t n_boxes, const double* lo, const double* hi, int dims, int64_t capacity_steps) {
    if (n_boxes < 0 || n_boxes > kMaxFlowBoxes) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_flow_enable: n_boxes out of range [0, 16]");
    if (n_boxes == 0) return;
    if (!lo || !hi) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_flow_enable: null table");
    if (capacity_steps < 1) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_flow_enable: capacity_steps must be positive");
    for (int64_t k = 0; k < (int64_t)n_boxes * dims; ++k) {
        if (std::isnan(lo[k]) || std::isnan(hi[k])) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_flow_enable: NaN bound");
        if (!(lo[k] < hi[k])) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_flow_enable: every box needs lo < hi on every axis");
    }
}

// sphmi_envelopes_enable: bit Type of the mask selects the rows of that Type (Fluid = 1, Fixed = 2, Moving = 3), as in
// sphmi_components_build; 0 disables; any other bit is an argument error
inline void check_envelope_mask(uint32_t type_mask) {
    if (type_mask & ~0xEu) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_envelopes_enable: type_mask has a bit other than 1 (Fluid), 2 (Fixed), 3 (Moving) set");
}

// sphmi_maps_enable: the argument errors; returns the number of bins.  An axis is collapsed by count 1 and spacing +inf; +inf with
// a count above 1 could hold no row beyond the first bin and is refused.
inline int64_t check_map_lattice(const double* origin, const double* spacing, const int64_t* counts, int dims, int32_t up_axis) {
    if (!origin || !spacing || !counts) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_maps_enable: null origin, spacing or counts");
    if (up_axis < 0 || up_axis >= dims) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_maps_enable: up_axis out of range [0, dims)");
    int64_t bins = 1;
    for (int d = 0; d < dims; ++d) {
        if (!std::isfinite(origin[d])) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_maps_enable: non-finite origin");
        if (std::isnan(spacing[d]) || !(spacing[d] > 0.0)) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_maps_enable: every spacing must be positive");
        if (counts[d] < 1) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_maps_enable: every count must be at least 1");
        if (std::isinf(spacing[d]) && counts[d] > 1) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_maps_enable: an infinite spacing collapses an axis and needs a count of 1");
        if (counts[d] > kMaxMapBins || bins * counts[d] > kMaxMapBins) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_maps_enable: more than SPHMI_MAX_MAP_BINS bins");
        bins *= counts[d];
    }
    return bins;
}
// … and the rows a handle may have: Σ llrint(v·2³²) over the rows of a bin stays inside an int64 while rows · max|v| < 2³¹; with
// |v| < 4·c₀ — a weakly compressible run keeps |v| near c₀ / 10 — that is rows <= 2³¹ / (4·c₀)
inline int64_t map_row_bound(double c0) {
    const double bound = 2147483648.0 / (4.0 * c0);
    return !(bound < 9.0e18) ? INT64_MAX : (int64_t)bound;
}

// sphmi_tracers_enable: the argument errors.  rows[] name the tracked particles in the row order of a download NOW (n_rows rows),
// positions[] hold `dims` doubles per drifter; both counts zero disables and nothing else is looked at.
inline void check_tracer_table(int32_t n_particles, const int64_t* rows, int64_t n_rows, int32_t n_drifters, const double* positions, int dims,
                               double min_weight, int64_t capacity_steps) {
    if (n_particles < 0 || n_particles > kMaxTracers) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_tracers_enable: n_particles out of range [0, 1024]");
    if (n_drifters < 0 || n_drifters > kMaxTracers) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_tracers_enable: n_drifters out of range [0, 1024]");
    if (n_particles == 0 && n_drifters == 0) return;
    if (n_particles > 0 && !rows) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_tracers_enable: null table of rows");
    if (n_drifters > 0 && !positions) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_tracers_enable: null table of positions");
    if (capacity_steps < 1) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_tracers_enable: capacity_steps must be positive");
    if (!std::isfinite(min_weight) || !(min_weight > 0.0)) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_tracers_enable: min_weight must be finite and positive");
    std::vector<int64_t> sorted;
    if (n_particles > 0) sorted.assign(rows, rows + n_particles);
    std::sort(sorted.begin(), sorted.end());
    for (int32_t k = 0; k < n_particles; ++k) {
        if (sorted[k] < 0 || sorted[k] >= n_rows) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_tracers_enable: row outside [0, n)");
        if (k > 0 && sorted[k] == sorted[k - 1]) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_tracers_enable: duplicate row");
    }
    for (int64_t k = 0; k < (int64_t)n_drifters * dims; ++k)
        if (!std::isfinite(positions[k])) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_tracers_enable: non-finite coordinate");
}

// sphmi_tracers_read: the payload { { x[3], v[3], ρ, P }[n_particles], { X[3], S, SP, Sρ, Sv[3], n }[n_drifters] } of the k-th
// delivered step, as recorded — the raw sums stay raw (a caller normalises them as sphmi_probes_read does, or moves a drifter again)
inline void deliver_tracers(int n_particles, int n_drifters, int64_t k, const double* v, double* particles, double* drifters) {
    const size_t np = (size_t)kTrParticleValues * n_particles, nd = (size_t)kTrDrifterValues * n_drifters;
    if (particles && np) memcpy(particles + (size_t)k * np, v, np * 8);
    if (drifters && nd) memcpy(drifters + (size_t)k * nd, v + np, nd * 8);
}

// sphmi_sample_grid: the argument errors every kind of handle reports alike; returns the number of nodes
inline int64_t check_grid_lattice(const double* origin, const double* spacing, const int64_t* counts, int dims) {
    if (!origin || !spacing || !counts) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_sample_grid: null origin, spacing or counts");
    int64_t nodes = 1;
    for (int d = 0; d < dims; ++d) {
        if (!std::isfinite(origin[d])) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_sample_grid: non-finite origin");
        if (!std::isfinite(spacing[d]) || !(spacing[d] > 0.0)) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_sample_grid: every spacing must be finite and positive");
        if (counts[d] < 1) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_sample_grid: every count must be at least 1");
        if (counts[d] > kMaxGridNodes || nodes * counts[d] > kMaxGridNodes) throw EngineError(SPHMI_ERR_ARGUMENT, "sphmi_sample_grid: more than SPHMI_MAX_GRID_NODES nodes");
        nodes *= counts[d];
    }
    return nodes;
}

// sphmi_sample_points, sphmi_sample_point_gradients and sphmi_sample_point_moments (`fn`): the argument errors every kind of handle reports alike
inline void check_sample_points(int64_t n_points, const double* positions, int dims, const char* fn = "sphmi_sample_points") {
    const std::string name(fn);
    if (n_points < 0 || n_points > kMaxSamplePoints) throw EngineError(SPHMI_ERR_ARGUMENT, name + ": n_points out of range [0, SPHMI_MAX_SAMPLE_POINTS]");
    if (n_points > 0 && !positions) throw EngineError(SPHMI_ERR_ARGUMENT, name + ": null positions");
    for (int64_t k = 0; k < n_points * dims; ++k)
        if (!std::isfinite(positions[k])) throw EngineError(SPHMI_ERR_ARGUMENT, name + ": non-finite coordinate at point " + std::to_string(k / dims));
}

// The series of an observer that records once per executed step: what the batches delivered since the last read, the newest
// `capacity` of it.  A sample carries the payload of a device-side record as it is (group forces: 3 per group; probes: the RAW
// sums, kPrValues per probe); what a read hands out of it is the caller's `deliver`.
struct StepSeries {
    struct Sample { int64_t iteration; double time, dt; std::vector<double> v; };
    int values = 0;                            // doubles of a payload
    int64_t capacity = 0, dropped = 0;
    std::deque<Sample> q;
    void reset(int values_per_step, int64_t cap) { values = values_per_step; capacity = cap; dropped = 0; q.clear(); }
    void push(Sample&& s) {
        if ((int64_t)q.size() >= capacity) { q.pop_front(); dropped += 1; }
        q.push_back(std::move(s));
    }
    // one record of a device-side log: `header` doubles { iteration (int64 bits), time, Δt, … }, then the payload
    static Sample decode(const double* rec, int header, int values) {
        Sample s{};
        memcpy(&s.iteration, rec, 8); s.time = rec[1]; s.dt = rec[2];
        s.v.assign(rec + header, rec + header + values);
        return s;
    }
    // a multi-device handle adds the slabs' records of a step, in slab order
    static void add(Sample& into, const Sample& other, const char* what) {
        if (other.iteration != into.iteration) throw EngineError(SPHMI_ERR_STATE, std::string(what) + ": the slabs' records of a step do not belong together");
        for (size_t c = 0; c < into.v.size(); ++c) into.v[c] += other.v[c];
    }
    // … or combines them slot by slot where not every slot is a sum: rule(slot) = 0 sum, 1 min, 2 max (bg_rule)
    template <class Rule>
    static void combine(Sample& into, const Sample& other, const char* what, Rule&& rule) {
        if (other.iteration != into.iteration) throw EngineError(SPHMI_ERR_STATE, std::string(what) + ": the slabs' records of a step do not belong together");
        for (size_t c = 0; c < into.v.size(); ++c) {
            const int r = rule((int)c);
            into.v[c] = r == 0 ? into.v[c] + other.v[c] : r == 1 ? std::fmin(into.v[c], other.v[c]) : std::fmax(into.v[c], other.v[c]);
        }
    }
    // the oldest min(cap, waiting) samples leave the series: deliver(k, payload) hands out the k-th of them
    template <class Deliver>
    void read(const char* fn_name, int64_t cap, int64_t* iteration, double* time, double* dt, int64_t* n_out, int64_t* n_dropped, Deliver&& deliver) {
        if (!n_out) throw EngineError(SPHMI_ERR_ARGUMENT, std::string(fn_name) + ": null n_out");
        if (cap < 0) throw EngineError(SPHMI_ERR_ARGUMENT, std::string(fn_name) + ": negative capacity");
        if (cap == 0) { *n_out = (int64_t)q.size(); if (n_dropped) *n_dropped = dropped; return; }      // a question: nothing is delivered, nothing cleared
        const int64_t n = std::min<int64_t>(cap, (int64_t)q.size());
        for (int64_t k = 0; k < n; ++k) {
            const Sample& s = q.front();
            if (iteration) iteration[k] = s.iteration;
            if (time) time[k] = s.time;
            if (dt) dt[k] = s.dt;
            deliver(k, s.v.data());
            q.pop_front();
        }
        *n_out = n;
        if (n_dropped) *n_dropped = dropped;
        dropped = 0;
    }
};

// sphmi_group_forces_read: the forces of the k-th delivered step, as recorded
inline void deliver_forces(int n_groups, int64_t k, const double* v, double* force) {
    if (force) memcpy(force + (size_t)k * 3 * n_groups, v, (size_t)3 * n_groups * 8);
}

// a mean of the kernel sums (probes and lattice alike); `some`: n > 0 && S > 0, else every value is 0
inline double kernel_mean(double sum, double S, bool some) { return some ? sum / S : 0.0; }

// sphmi_probes_read: the raw sums { S, SP, Sρ, Sv[3], n } of the k-th delivered step, normalised
inline void deliver_probe_means(int n_probes, int64_t k, const double* sums, double* weight, int64_t* count, double* pressure, double* density, double* velocity) {
    for (int p = 0; p < n_probes; ++p) {
        const double* v = sums + (size_t)kPrValues * p;
        const size_t at = (size_t)k * n_probes + p;
        const bool some = v[6] > 0.0 && v[0] > 0.0;
        if (weight) weight[at] = v[0];
        if (count) count[at] = (int64_t)v[6];
        if (pressure) pressure[at] = kernel_mean(v[1], v[0], some);
        if (density) density[at] = kernel_mean(v[2], v[0], some);
        if (velocity) for (int d = 0; d < 3; ++d) velocity[3 * at + d] = kernel_mean(v[3 + d], v[0], some);
    }
}

// sphmi_budgets_read: what turns the raw budgets into energies and momenta.  B = c₀²ρ₀/7 is the Cb/γ of the Tait equation the
// engine runs (γ = 7); the kernels record Σ e(ρ) in units of B/ρ₀.
struct BudgetFactors {
    double mass, potential, internal;          // m₀,  m₀·g,  m₀·(B/ρ₀)
    BudgetFactors(double m0, double g, double c0, double rho0) : mass(m0), potential(m0 * g), internal(m0 * (((c0 * c0 * rho0) / 7.0) / rho0)) {}
};
// … the raw record { n, Σ½v², Σx_last, Σe, Σv[3], Σx×v[3], Σx[3], max v², min ρ, max ρ, min x[3], max x[3] } of the k-th delivered
// step: one multiplication or division per value; a step without Fluid rows (n = 0: ±inf in the extremes) delivers zeros
inline void deliver_budgets(const BudgetFactors& f, int64_t k, const double* v, int64_t* count, double* energy, double* momentum, double* angular,
                            double* centre, double* extremes, double* box) {
    const bool some = v[0] > 0.0;
    if (count) count[k] = (int64_t)v[0];
    if (energy) { energy[3 * k] = f.mass * v[1]; energy[3 * k + 1] = f.potential * v[2]; energy[3 * k + 2] = f.internal * v[3]; }
    if (momentum) for (int d = 0; d < 3; ++d) momentum[3 * k + d] = f.mass * v[4 + d];
    if (angular) for (int d = 0; d < 3; ++d) angular[3 * k + d] = f.mass * v[7 + d];
    if (centre) for (int d = 0; d < 3; ++d) centre[3 * k + d] = some ? v[10 + d] / v[0] : 0.0;
    if (extremes) { extremes[3 * k] = some ? std::sqrt(v[13]) : 0.0; extremes[3 * k + 1] = some ? v[14] : 0.0; extremes[3 * k + 2] = some ? v[15] : 0.0; }
    if (box) for (int d = 0; d < 6; ++d) box[6 * k + d] = some ? v[16 + d] : 0.0;
}

// sphmi_flow_read: the raw record { n_after, Σ1/ρ, Σv[3], entered, left } per box of the k-th delivered step: the counts as they are
// (exact integers carried in doubles), volume and momentum one multiplication by m₀ each
inline void deliver_flow(double m0, int n_boxes, int64_t k, const double* raw, int64_t* count, double* volume, double* momentum, int64_t* entered,
                         int64_t* left) {
    for (int b = 0; b < n_boxes; ++b) {
        const double* v = raw + (size_t)kFlValues * b;
        const size_t at = (size_t)k * n_boxes + b;
        if (count) count[at] = (int64_t)v[0];
        if (volume) volume[at] = m0 * v[1];
        if (momentum) for (int d = 0; d < 3; ++d) momentum[3 * at + d] = m0 * v[2 + d];
        if (entered) entered[at] = (int64_t)v[5];
        if (left) left[at] = (int64_t)v[6];
    }
}

// sphmi_envelopes_read: the window header as the device keeps it { steps (int64 bits), t_begin, t_end, duration } → the caller's
// steps_out and window_out[3]
inline void deliver_envelope_window(const double* header, int64_t* steps_out, double* window_out) {
    if (steps_out) memcpy(steps_out, header, 8);
    if (window_out) for (int k = 0; k < 3; ++k) window_out[k] = header[1 + k];
}
// … and the largest speed of every row from max |v|² (slot 6), in place: the one sqrt, on the host (NaN stays NaN)
inline void deliver_envelope_speed(int64_t n, double* speed) {
    if (speed) for (int64_t i = 0; i < n; ++i) speed[i] = std::sqrt(speed[i]);
}

// sphmi_maps_read: three arrays of one component each, as the device keeps them, → the caller's [bins][3]
inline void deliver_map_vectors(int64_t bins, const double* c0, const double* c1, const double* c2, double* out) {
    if (out) for (int64_t b = 0; b < bins; ++b) { out[3 * b] = c0[b]; out[3 * b + 1] = c1[b]; out[3 * b + 2] = c2[b]; }
}

// The samplers that hand their kernel sums out RAW state their layout HERE and nowhere else on the host: one { first slot, width }
// per caller-visible output, in the order of the C prototype.  Slot 0 (S → weight_out) and slot 6 (n → count_out, as an integer)
// are not in a table: every sampler has them.  The store statements of k_point_gradients and k_point_moments fill these slots.
struct OutputSlots { int first, width; };
constexpr OutputSlots kPgOutputs[] = {{1, 1}, {2, 1}, {3, 3},          // sum_pressure, sum_density, sum_velocity: the cloud's
                                      {7, 3}, {10, 3}, {13, 3}, {16, 9}}; // grad_weight, grad_pressure, grad_density, grad_velocity
constexpr OutputSlots kPmOutputs[] = {{1, 1}, {2, 1}, {3, 3},          // sum_pressure, sum_density, sum_velocity: the cloud's
                                      {7, 3}, {10, 6},                  // moment1, moment2
                                      {16, 3}, {19, 3}, {22, 9}};       // moment_pressure, moment_density, moment_velocity
constexpr int kRawOutputsMax = 8;
// a table tiles [1, values) in order, without gap or overlap, around slot 6
template <int N> constexpr bool outputs_tile(const OutputSlots (&t)[N], int values) {
    int at = 1;
    for (int i = 0; i < N; ++i) {
        if (at == 6) at = 7;
        if (t[i].first != at || t[i].width < 1 || (at < 6 && at + t[i].width > 6)) return false;
        at += t[i].width;
    }
    return at == values;
}
static_assert(outputs_tile(kPgOutputs, kPgValues), "the outputs of sphmi_sample_point_gradients tile the slots of k_point_gradients");
static_assert(outputs_tile(kPmOutputs, kPmValues), "the outputs of sphmi_sample_point_moments tile the slots of k_point_moments");

struct GridSums;
// the caller's pointers of one such call, out[] in table order (any may be null)
struct RawOutputs {
    const OutputSlots* table;
    int entries, values;
    double* weight;
    int64_t* count;
    double* out[kRawOutputsMax];
    template <int N> RawOutputs(const OutputSlots (&t)[N], double* weight_out, int64_t* count_out, double* const (&outputs)[N])
        : table(t), entries(N), values(t[N - 1].first + t[N - 1].width), weight(weight_out), count(count_out), out{} {
        static_assert(N <= kRawOutputsMax, "RawOutputs holds at most kRawOutputsMax pointers");
        for (int i = 0; i < N; ++i) out[i] = outputs[i];
    }
    // the slots of `values` the outputs need → w[values]
    void wanted(bool* w) const {
        w[0] = weight != nullptr; w[6] = count != nullptr;
        for (int i = 0; i < entries; ++i)
            for (int c = 0; c < table[i].width; ++c) w[table[i].first + c] = out[i] != nullptr;
    }
    inline void deliver(const GridSums& G) const;
};
// … and the five outputs of the lattice and the cloud, which GridSums turns into means: constructed from and delivered like
// RawOutputs, so that one call path serves both kinds (EngineBase::sample)
struct MeanOutputs {
    double* weight; int64_t* count; double *pressure, *density, *velocity;
    inline void deliver(const GridSums& G) const;
};

// The host side of sphmi_sample_grid and sphmi_sample_points: the raw sums { S, SP, Sρ, Sv[3], n } of the lattice
// (sphmi_field_grid.h) or the cloud (sphmi_point_cloud.h), `nodes` of either, the ones the requested outputs need.  S lands in weight_out itself when that is asked for; the means are formed here, 0 where n == 0.
// sphmi_sample_point_gradients (sphmi_point_gradients.h) and sphmi_sample_point_moments (sphmi_point_moments.h) carry `values` =
// kPgValues / kPmValues sums per point in the same arrays — the first seven are the cloud's — and hand them out RAW (the second
// constructor, RawOutputs::deliver): a multi-device handle adds both kinds with one loop.
struct GridSums {
    int64_t nodes = 0;
    int values = kFgValues;                    // sums per node
    double* S = nullptr;                       // weight_out, or s[0]
    std::vector<double> s[kSampleValuesMax];
    bool want[kSampleValuesMax] = {};
    double* dst(int f) { return f == 0 ? S : s[f].data(); }
    GridSums(int64_t n, double* weight, const int64_t* count, const double* pressure, const double* density, const double* velocity) : nodes(n) {
        const bool means = pressure || density || velocity;
        want[0] = weight || means; want[1] = pressure != nullptr; want[2] = density != nullptr;
        want[3] = want[4] = want[5] = velocity != nullptr; want[6] = count || means;
        for (int f = 0; f < kFgValues; ++f) if (want[f] && !(f == 0 && weight)) s[f].assign((size_t)n, 0.0);
        S = weight ? weight : s[0].data();
    }
    GridSums(int64_t n, const MeanOutputs& o) : GridSums(n, o.weight, o.count, o.pressure, o.density, o.velocity) {}
    void deliver(int64_t* count, double* pressure, double* density, double* velocity) const {
        const double* n = s[6].data();
        for (int64_t k = 0; k < nodes; ++k) {
            if (count) count[k] = (int64_t)n[k];
            if (!pressure && !density && !velocity) continue;
            const bool some = n[k] > 0.0 && S[k] > 0.0;
            if (pressure) pressure[k] = kernel_mean(s[1][k], S[k], some);
            if (density) density[k] = kernel_mean(s[2][k], S[k], some);
            if (velocity) for (int d = 0; d < 3; ++d) velocity[3 * k + d] = kernel_mean(s[3 + d][k], S[k], some);
        }
    }
    // the raw sums of the gradients or the moments: the slots the outputs' table asks for; S goes straight into weight_out
    GridSums(int64_t n, const RawOutputs& out) : nodes(n), values(out.values) {
        out.wanted(want);
        for (int f = 0; f < values; ++f) if (want[f] && !(f == 0 && out.weight)) s[f].assign((size_t)n, 0.0);
        S = out.weight ? out.weight : s[0].data();
    }
    // the wanted sums in slot order: f(slot, where it goes)
    template <class F> void for_wanted(F&& f) {
        for (int k = 0; k < values; ++k) if (want[k]) f(k, dst(k));
    }
};
static_assert(kPgValues <= kSampleValuesMax && kPmValues <= kSampleValuesMax, "GridSums holds at most kSampleValuesMax sums per node");

// n → count_out as an integer; the slots of every other output → [nodes × width], as they are
inline void RawOutputs::deliver(const GridSums& G) const {
    if (count) for (int64_t k = 0; k < G.nodes; ++k) count[k] = (int64_t)G.s[6][k];
    for (int i = 0; i < entries; ++i) {
        if (!out[i]) continue;
        const int width = table[i].width;
        for (int c = 0; c < width; ++c) {
            const double* v = G.s[table[i].first + c].data();
            for (int64_t k = 0; k < G.nodes; ++k) out[i][(size_t)width * k + c] = v[k];
        }
    }
}
inline void MeanOutputs::deliver(const GridSums& G) const { G.deliver(count, pressure, density, velocity); }

// sphmi_probe_moments_read: the raw sums of the k-th delivered step — kPmValues slots per probe, probe-major, as k_probe_moments
// records them — → the caller's [capacity × n_probes × width] arrays, as they are; n → count_out as an integer.  `out` is built over
// kPmOutputs: the layout is stated there and nowhere else.
inline void deliver_probe_moments(int n_probes, int64_t k, const double* sums, const RawOutputs& out) {
    for (int p = 0; p < n_probes; ++p) {
        const double* v = sums + (size_t)out.values * p;
        const size_t at = (size_t)k * n_probes + p;
        if (out.weight) out.weight[at] = v[0];
        if (out.count) out.count[at] = (int64_t)v[6];
        for (int i = 0; i < out.entries; ++i) {
            if (!out.out[i]) continue;
            const int width = out.table[i].width;
            for (int c = 0; c < width; ++c) out.out[i][(size_t)width * at + c] = v[out.table[i].first + c];
        }
    }
}

}  // namespace sphmi
