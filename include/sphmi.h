/*
 * sphmi.h — C ABI of the MI355X-native SPH neighbour + force engine (libsphmi.so).
 *
 * This is the drop-in boundary for the hot path of AhmedSalih3d/SPHExample: one call to
 * sphmi_advance() replaces one call to the reference's
 *     SimulationLoop(...)                      src/SPHCellList.jl:727-805 (called at :883)
 * i.e. "advance the particle system until TotalTime > next_output_time", including the
 * cell-list rebuild (UpdateNeighbors!, :138-163), both neighbour passes
 * (NeighborLoop!/ComputeInteractions!, :168-217 / :268-317), mDBC (:219-266, :319-365, :598-622),
 * the predictor / corrector (HalfTimeStep :624-638, FullTimeStep :640-652, DensityEpsi!,
 * LimitDensityAtBoundary!, Pressure!  src/SimulationEquations.jl:9-42) and the adaptive time step
 * (src/TimeStepping.jl:24-46, update_delta_x! src/SPHCellList.jl:706-724).
 *
 * Conventions
 *   - plain C, no C++ types, no exceptions cross the boundary; every function returns an int
 *     status (SPHMI_OK == 0) and sphmi_last_error() gives the text of the last failure.
 *   - the caller owns every host array it passes; pointers only need to stay valid for the
 *     duration of the call (Julia: GC.@preserve around the ccall).  The engine owns all device
 *     memory behind the opaque handle.
 *   - vector fields cross the boundary exactly as Julia lays out Vector{SVector{D,T}}:
 *     contiguous AoS, D components interleaved, N*D scalars.
 *   - host scalars are `host_float_bytes` wide (8 for every stock example), device arithmetic is
 *     `device_float_bytes` wide (4 = fp32 kernels, 8 = fp64 kernels, 0 = the library chooses:
 *     sphmi_auto_device_float_bytes); conversion happens in upload/download.
 *   - the library installs no signal handlers and never calls back into the host runtime.
 *   - one handle = one simulation; a handle must not be used from two threads at once.  A handle created with a
 *     device list (sphmi_config.n_devices > 1) spreads the simulation over the GPUs of the node — slabs of the domain,
 *     one-cell halo over RCCL/xGMI each neighbour pass — behind the SAME sphmi_upload / sphmi_advance / sphmi_download
 *     calls: the caller (one Julia process, src/SPHCellList.jl:883) does not change.
 */
#ifndef SPHMI_H
#define SPHMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPHMI_ABI_VERSION 5
#define SPHMI_MAX_DEVICES 16
#define SPHMI_MAX_COLUMNS 16
#define SPHMI_MAX_COLUMN_ROW_BYTES 64
#define SPHMI_MAX_FORCE_GROUPS 16
#define SPHMI_MAX_PROBES 1024

/* status codes */
enum {
    SPHMI_OK              = 0,
    SPHMI_ERR_ARGUMENT    = 1,  /* bad config / null pointer / unsupported model tag          */
    SPHMI_ERR_DEVICE      = 2,  /* HIP runtime failure (text in sphmi_last_error)              */
    SPHMI_ERR_NUMERIC     = 3,  /* NaN / non-positive dt produced by the time-step criterion   */
    SPHMI_ERR_DOMAIN      = 4,  /* bounding cell grid exceeds the configured cell budget       */
    SPHMI_ERR_STATE       = 5   /* call sequence error (e.g. advance before upload)            */
};

/* model tags; values mirror the reference's dispatch types */
enum { SPHMI_KERNEL_WENDLAND_C2 = 0, SPHMI_KERNEL_CUBIC_SPLINE = 1 };   /* src/SPHKernels.jl:13-19,75-126 */
enum { SPHMI_KOUT_NONE = 0, SPHMI_KOUT_STORE = 1 };         /* KMode: src/SPHCellList.jl:90-116 */
enum { SPHMI_VISC_ZERO = 0, SPHMI_VISC_ARTIFICIAL = 1, SPHMI_VISC_LAMINAR = 2, SPHMI_VISC_LAMINAR_SPS = 3 };
                                                            /* src/SPHViscosityModels.jl:51-126  */
enum { SPHMI_DDT_NONE = 0, SPHMI_DDT_ZERO_GRAVITY_LINEAR = 1, SPHMI_DDT_LINEAR = 2, SPHMI_DDT_COMPLEX = 3 };
                                                            /* src/SPHDensityDiffusionModels.jl:30-188 */
enum { SPHMI_SHIFT_NONE = 0, SPHMI_SHIFT_PLANAR = 1 };      /* src/SPHCellList.jl:73-88,654-677 */
enum { SPHMI_MDBC_NONE = 0, SPHMI_MDBC_SIMPLE = 1 };        /* src/SimulationMetaDataConfiguration.jl:20-22 */
/* ParticleType values, src/SimulationGeometry.jl:10-14 */
enum { SPHMI_FLUID = 1, SPHMI_FIXED = 2, SPHMI_MOVING = 3 };

/*
 * Parameter block = the fields of SimulationConstants (src/SimulationConstantsConfiguration.jl:36-52)
 * and SPHKernelInstance (src/SPHKernels.jl:30-72) passed by value, plus the type parameters of
 * SimulationMetaData{D,T,SMode,KMode,BMode,LMode} (src/SimulationMetaDataConfiguration.jl:28-33)
 * and the model tag types as enums.
 */
typedef struct sphmi_config {
    int32_t struct_size;         /* = sizeof(sphmi_config); ABI guard                            */
    int32_t abi_version;         /* = SPHMI_ABI_VERSION                                          */
    int32_t dims;                /* Dimensions: 2 or 3                                           */
    int32_t host_float_bytes;    /* FloatType of the host arrays: 4 or 8                         */
    int32_t device_float_bytes;  /* arithmetic type of the kernels: 4, 8, or 0 = chosen by the library (sphmi_auto_device_float_bytes) */
    int32_t kernel;              /* SPHMI_KERNEL_*                                               */
    int32_t viscosity;           /* SPHMI_VISC_*                                                 */
    int32_t density_diffusion;   /* SPHMI_DDT_*                                                  */
    int32_t mdbc;                /* SPHMI_MDBC_*                                                 */
    int32_t device;              /* HIP device ordinal                                           */
    int32_t shifting;            /* SPHMI_SHIFT_* (SMode of SimulationMetaData)                  */
    int32_t kernel_output;       /* SPHMI_KOUT_* (KMode of SimulationMetaData)                   */
    int64_t n_particles;         /* length(SimParticles); below 2^27 (fp32 kernels) / 2^26 (fp64) per device: 32-bit gather offsets */
    int64_t max_cells;           /* cell budget of the dense bounding grid; 0 = default (1<<30: two 4-byte arrays with 25 % headroom, 10.7 GB at the limit, allocated on demand; SPHMI_ERR_DOMAIN when the device cannot hold them) */
    /* SimulationConstants */
    double rho0, dx, m0, alpha, g, c0, gamma, delta_phi, CFL, Cb, nu0;
    /* SPHKernelInstance */
    double k, h, h_inv, H, H_inv, H2, alphaD, eta2;
    /* SimulationConstants, continued (LaminarSPS) */
    double blin_constant, smagorinsky_constant;
    /* CubicSpline.eps (tensile correction, src/SPHKernels.jl:15-19,114-126) */
    double cubic_eps;
    /* Device list: n_devices <= 1 → one GPU, `device` above.  n_devices > 1 → the particle set is
     * split into n_devices slabs along one axis, slab r on HIP device devices[r]; halos and the per-step MAX-allreduce
     * travel over RCCL.  The same ordinal may appear more than once (several slabs share that GPU; transfers are then
     * stream-ordered device copies — the single-GPU test configuration).  slab_axis: 0 = chosen for balance, 1 / 2 / 3 =
     * x / y / z. */
    int32_t n_devices;
    int32_t slab_axis;
    int32_t devices[SPHMI_MAX_DEVICES];
} sphmi_config;

/* What the reference's SimulationLoop leaves in SimMetaData (src/SPHCellList.jl:679-685,:759). */
typedef struct sphmi_progress {
    int64_t iteration;        /* SimMetaData.Iteration                                            */
    int64_t steps_done;       /* steps executed by this call                                      */
    int64_t n_rebuilds;       /* UpdateNeighbors! executions since create                         */
    int64_t index_counter;    /* SimMetaData.IndexCounter = 1 + number of occupied cells          */
    double  total_time;       /* SimMetaData.TotalTime                                            */
    double  last_dt;          /* SimMetaData.CurrentTimeStep                                      */
    double  delta_x;          /* the loop-local Δx accumulator (src/SPHCellList.jl:739,744,760)   */
} sphmi_progress;

typedef struct sphmi_handle sphmi_handle;

/* Library identification: "sphmi <abi> hip gfx950 ..." — static string. */
const char* sphmi_backend_info(void);

/* Text of the last error on this handle (or of the last failed sphmi_create when h == NULL). */
const char* sphmi_last_error(const sphmi_handle* h);

/* Allocate device state for cfg->n_particles particles.  Replaces the allocations at
 * src/SPHCellList.jl:825,837,840-844 (support arrays, per-thread copies, ParticleRanges,
 * UniqueCells, CellDict, sort scratch). */
int sphmi_create(const sphmi_config* cfg, sphmi_handle** out);

/* The arithmetic `device_float_bytes = 0` resolves to for this configuration: 4 (fp32 kernels, double-float state) when every term of
 * the path is continuous in the positions — the kernel support ends where the kernel and its gradient vanish (H >= 2h, the default
 * k = 2 of src/SPHKernels.jl:57-60, so nothing jumps at the r^2 <= H^2 cut of src/SPHCellList.jl:275) and there is no mDBC; 8 (fp64
 * kernels) when the kernel is cut off before it vanishes (k < 2: example/DucklingMDBC.jl, example/MovingSquare2d.jl) or mDBC is on
 * (src/SPHCellList.jl:598-622: "no neighbour -> keep", the Shepard fallback and the |det A| >= 1e-3 switch are discontinuities) — there
 * an fp32 trajectory takes the other branch a step early or late and leaves the reference's state by more than 1e-5 on single
 * particles.  ("H >= 2h" is tested with a relative slack of 1e-12: H = k*h is formed in floating point on the caller's side.)  A handle too
 * large for the fp64 kernels (more than 2^26 - 1 particles per device) stays with fp32 whatever the policy says.
 * sphmi_device_float_bytes: what a handle runs. */
int32_t sphmi_auto_device_float_bytes(const sphmi_config* cfg);
int sphmi_device_float_bytes(const sphmi_handle* h, int32_t* device_float_bytes_out);
int sphmi_destroy(sphmi_handle* h);

/*
 * Copy the SimParticles fields the hot path reads (src/PreProcess.jl:114) to the device.
 * position / velocity / acceleration / ghost_points: N*D host floats (AoS); density: N host floats;
 * type: N ParticleType bytes; id: N Int64; group_marker: N UInt64 (may be NULL);
 * ghost_points may be NULL when mdbc == SPHMI_MDBC_NONE.  GravityFactor / MotionLimiter are
 * derived from `type` exactly as src/PreProcess.jl:78-98 does.
 * Also resets Positionₙ⁺ to zero as AllocateSupportDataStructures does (src/PreProcess.jl:131).
 */
int sphmi_upload(sphmi_handle* h,
                 const void* position, const void* velocity, const void* acceleration,
                 const void* density, const uint8_t* type, const int64_t* id,
                 const uint64_t* group_marker, const void* ghost_points);

/*
 * Pre-processing on the device for the case the headline is quoted on.  The reference builds
 * SimParticles from CSV point lists (LoadSpecificCSV / AllocateDataStructures, src/PreProcess.jl:45-119) and ships the
 * 3-D dam break only at Dp 0.02; sphmi_generate_dam_break_3d fills the handle with the lattice of that case at any
 * spacing dp — same node set, order, IDs (1 … N, boundary first), Type / GroupMarker and hydrostatic densities as the
 * files (and as the host generator the tests compare with) — without host arrays or an upload, and leaves the handle
 * in the state sphmi_upload leaves it in.  cfg->n_particles must equal n_bound + n_fluid of sphmi_dam_break_3d_count;
 * rho0, g, c0 come from the handle's config.  3-D single-device handles.
 */
int sphmi_dam_break_3d_count(double dp, int64_t* n_bound_out, int64_t* n_fluid_out);
int sphmi_generate_dam_break_3d(sphmi_handle* h, double dp);

/* Set / read SimMetaData.Iteration and SimMetaData.TotalTime (they live in the host struct). */
int sphmi_set_clock(sphmi_handle* h, int64_t iteration, double total_time);

/*
 * Output without stalling the run: sphmi_download_begin snapshots the requested fields on the
 * device in stream order and starts the device→host copies on a second stream; the caller may call sphmi_advance
 * right away and must not touch the host arrays until sphmi_download_end returns.  sphmi_download = begin + end.
 * sphmi_host_register page-locks a host array the caller will hand in again and again (the fields of the
 * StructArray live for the whole run): registered arrays are written by the copy engine WHILE the caller advances;
 * arrays that are not registered are filled from the device-side snapshot inside sphmi_download_end, through a
 * page-locked bounce buffer of the handle (the library never hands a pageable pointer to the runtime: its cached pins
 * of the caller's pages go stale when the allocator re-uses the addresses).  The contract is the same either way: the
 * arrays hold the snapshot when sphmi_download_end returns.  The caller must unregister (or destroy the handle) before
 * freeing a registered array.
 */
int sphmi_download_begin(sphmi_handle* h,
                         void* position, void* velocity, void* acceleration, void* density, void* pressure,
                         int64_t* id, uint8_t* type, uint64_t* group_marker, void* ghost_points, int64_t* cells);
int sphmi_download_end(sphmi_handle* h);
/* Components per vector of the downloaded Position / Velocity / Acceleration / GhostPoints: `dims` (default, the
 * SVector{D} layout of SimParticles) or 3 — the point layout of the VTKHDF writer, which pads 2-D vectors with a zero
 * (to_3d!, src/ProduceHDFVTK.jl:251-325): the arrays handed to sphmi_download* then hold n×3 values and can be appended
 * to the `Points` / PointData datasets as they are.  Cells stay n×dims. */
int sphmi_set_output_components(sphmi_handle* h, int components);
/* (multi-device handles stage through page-locked buffers of their own and merge the slabs on the host: registering the
 * caller's arrays is accepted and gains nothing there) */
int sphmi_host_register(sphmi_handle* h, void* ptr, int64_t bytes);
int sphmi_host_unregister(sphmi_handle* h, void* ptr);

/*
 * StoreKernelOutput (src/SPHCellList.jl:106-116): Kernel[i] = Σⱼ Wᵢⱼ and KernelGradient[i] = Σⱼ ∇ᵢWᵢⱼ of the last
 * neighbour pass (the corrector of the last executed step, or the pass of sphmi_forces_once), host float type, n and n×dims values, current (cell-sorted) order.  Needs kernel_output = STORE.
 */
int sphmi_download_kernel_output(sphmi_handle* h, void* kernel, void* kernel_gradient);

/*
 * The sort as a permutation.  The reference's sort! permutes ALL 17 fields of the SimParticles StructArray
 * (src/SPHCellList.jl:142); the engine carries the ten the hot path touches and sphmi_download returns those in the
 * current cell-sorted order.  prev_row (N Int64, 0-based) says where every row came from: row i of the arrays
 * sphmi_download delivers NOW was row prev_row[i] at the previous call of sphmi_download_permutation (at sphmi_upload
 * for the first call), so the caller brings the fields the engine does not carry (GhostNormals, ChunkID, user columns)
 * along with ONE gather per field — no sort on the host.  The engine has the permutation from its own sort (a 4-byte
 * column that travels with the particles); multi-device handles derive it from the ID column.  Not for rank-mode handles.
 */
int sphmi_download_permutation(sphmi_handle* h, int64_t* prev_row);

/*
 * The caller's passive columns on the device: the fields of the StructArray the engine does not carry (ChunkID, GravityFactor,
 * MotionLimiter, BoundaryBool, GhostNormals, Kernel / KernelGradient without StoreKernelOutput) and any user column, attached
 * once and delivered with every output in the current cell-sorted order — the permutation never visits the host.
 *   attach: after sphmi_upload / sphmi_generate_dam_break_3d, at any later time too.  columns[c] holds n_particles x row_bytes[c]
 *     opaque bytes; row r belongs to the particle that is row r of what sphmi_download would deliver NOW.  The data are copied: the
 *     caller may free them on return.  1 <= row_bytes[c] <= SPHMI_MAX_COLUMN_ROW_BYTES (any value), n_columns <= SPHMI_MAX_COLUMNS.
 *     A second call replaces the set, n_columns = 0 detaches; sphmi_upload and the generator detach (a new particle set).
 *   download: columns_out[c] receives column c in the current order; a NULL entry skips that column.  begin / end, page-locked
 *     (sphmi_host_register) against bounce-buffer targets: exactly as sphmi_download_begin.  sphmi_download_columns_begin may be
 *     called on its own or directly after sphmi_download_begin; it then neither completes nor waits for the pending field
 *     download: both snapshots are taken in stream order with no step between them — row i of every column is the particle of
 *     row i of every field — and ONE sphmi_download_end completes both.  sphmi_download_columns = begin + sphmi_download_end.
 *   sphmi_download_permutation is independent: called any number of times or never, it does not change what the columns
 *     deliver, and a column download does not move its epoch.
 *   SPHMI_ERR_STATE: before the upload; download with nothing attached; rank-mode handles (a process holds one slab of the rows).
 *   SPHMI_ERR_ARGUMENT: null table, n_columns or a row_bytes out of range, a null column in attach.
 * Multi-device handles of one process keep the attached columns on the host (they merge every download there anyway).
 */
int sphmi_attach_columns(sphmi_handle* h, int32_t n_columns, const void* const* columns, const int32_t* row_bytes);
int sphmi_download_columns_begin(sphmi_handle* h, void* const* columns_out);
int sphmi_download_columns(sphmi_handle* h, void* const* columns_out);

/*
 * The force on particle groups at STEP resolution, recorded on the device: the drag on a moving body, the impact load on a wall — an
 * integrated load whose peaks last a few steps where an output interval has hundreds.  For every executed step and every selected
 * GroupMarker g
 *     F_g = m0 * sum of Acceleration[i] over the rows i of the handle with GroupMarker[i] == g
 * with Acceleration what sphmi_download would deliver directly after that step (the corrector's value, gravity included; the reference
 * writes it for boundary particles too).  The sum is formed in fp64 on fp32 and fp64 handles alike, in an order that depends on the
 * particle order alone: repeated runs give the same bits.  Off by default; a handle that never enables it launches what it always did.
 *   enable: after sphmi_upload / sphmi_generate_dam_break_3d, at any later time too.  1 <= n_groups <= SPHMI_MAX_FORCE_GROUPS distinct
 *     markers; a marker no particle carries is legal and yields zeros.  The handle keeps the newest capacity_steps (>= 1) samples that
 *     have not been read.  A second call replaces the selection and drops the series; n_groups = 0 disables.  sphmi_upload and the
 *     generator disable (a new particle set), as they detach the columns.  No step waits for the host: the records of a batch of
 *     queued steps come back with the control block the host fetches anyway.  sphmi_forces_once records nothing.
 *   read: delivers and clears the oldest `capacity` samples recorded since the last read, oldest first: iteration_out / time_out / dt_out
 *     [capacity] receive SimMetaData.Iteration, TotalTime (at the END of the step) and the step's dt exactly as sphmi_progress reports them
 *     after that step, force_out [capacity x n_groups x 3] the forces (2-D handles: a zero third component); any of the four may be NULL.
 *     *n_out: samples delivered; *n_dropped (may be NULL): samples lost since the last read because more than capacity_steps had
 *     accumulated (the oldest go).  capacity = 0 asks: *n_out = samples waiting, nothing is delivered or cleared.
 *   SPHMI_ERR_STATE: before the upload; read while disabled; rank-mode handles (a process holds one slab of the rows).
 *   SPHMI_ERR_ARGUMENT: null table, n_groups out of range, duplicate markers, capacity_steps < 1, null n_out.
 * Multi-device handles of one process: every slab sums the rows it owns (ghost copies do not count) and the handle adds the slabs'
 * records in slab order.
 */
int sphmi_group_forces_enable(sphmi_handle* h, int32_t n_groups, const uint64_t* markers, int64_t capacity_steps);
int sphmi_group_forces_read(sphmi_handle* h, int64_t capacity, int64_t* iteration_out, double* time_out, double* dt_out,
                            double* force_out, int64_t* n_out, int64_t* n_dropped);

/*
 * Pressure, density and velocity at fixed PROBE points at STEP resolution, recorded on the device: the pressure sensors on an obstacle,
 * the columns of points of a water-height gauge.  For every executed step and every probe p at x_p (`dims` doubles), over the rows j of
 * the handle with Type == Fluid and |x_p - x_j|^2 <= H^2 on the state sphmi_download would deliver directly after that step:
 *     w_j = (m0 / rho_j) * W(|x_p - x_j|)     W: the handle's kernel (Wendland C2 or CubicSpline, its alphaD and h)
 *     n = number of such rows    S = sum w_j    SP = sum w_j P_j    Srho = sum w_j rho_j    Sv = sum w_j v_j
 * A probe is not a particle: there is no self term and r = 0 is legal.  The sums cover EVERY Fluid row within H of the probe on the
 * current positions, however long ago the cell list was rebuilt (the pair loop's stale lists, quirk Q1, are not reproduced here).  They
 * are formed in fp64 on fp32 and fp64 handles alike, in an order that depends on the particle order alone: repeated runs give the same
 * bits.  Off by default; a handle that never enables it launches what it always did.
 *   enable: after sphmi_upload / sphmi_generate_dam_break_3d, at any later time too.  1 <= n_probes <= SPHMI_MAX_PROBES finite points,
 *     positions[n_probes x dims]; a probe in empty space or outside the particles' bounding grid is legal and yields zeros.  The handle
 *     keeps the newest capacity_steps (>= 1) samples that have not been read.  A second call replaces the set and drops the series;
 *     n_probes = 0 disables.  sphmi_upload and the generator disable.  No step waits for the host: the records of a batch of queued
 *     steps come back with the control block the host fetches anyway.  sphmi_forces_once records nothing.
 *   read: delivers and clears the oldest `capacity` samples recorded since the last read, oldest first: iteration_out / time_out / dt_out
 *     [capacity] as sphmi_group_forces_read; weight_out [capacity x n_probes] S, count_out [capacity x n_probes] n, pressure_out /
 *     density_out [capacity x n_probes] SP / S and Srho / S, velocity_out [capacity x n_probes x 3] Sv / S (2-D handles: a zero third
 *     component) - normalised on the host from the raw sums, 0 where n == 0.  S is the Shepard sum: ~1 inside the fluid, ~1/2 at a
 *     free surface, 0 in empty space (a water level is the height at which S crosses a threshold along a column of probes).  Any output
 *     pointer may be NULL.  *n_out, *n_dropped, capacity = 0: as sphmi_group_forces_read.
 *   SPHMI_ERR_STATE: before the upload; read while disabled; rank-mode handles (a process holds one slab of the rows); handles with H < h.
 *   SPHMI_ERR_ARGUMENT: null table, n_probes out of range, a non-finite coordinate, capacity_steps < 1, null n_out.
 * Multi-device handles of one process: every slab sums the rows it owns for every probe (ghost copies do not count), the handle adds the
 * slabs' raw sums in slab order and then normalises.  Probes and group forces may be enabled together.
 */
int sphmi_probes_enable(sphmi_handle* h, int32_t n_probes, const double* positions /* n_probes x dims */, int64_t capacity_steps);
int sphmi_probes_read(sphmi_handle* h, int64_t capacity, int64_t* iteration_out, double* time_out, double* dt_out,
                      double* weight_out, int64_t* count_out, double* pressure_out, double* density_out, double* velocity_out,
                      int64_t* n_out, int64_t* n_dropped);

/*
 * The global BUDGETS of the fluid at STEP resolution, recorded on the device: the energy, momentum and extent curves of a run - the
 * wave front of a dam break, the largest speed and the density extremes that show first when a run goes unstable.  For every executed
 * step, over the rows i of the handle with Type == Fluid, on the state sphmi_download would deliver directly after that step (x, v, rho
 * the doubles of that download; 2-D handles: z = 0, vz = 0), the raw values
 *     s0 = n, the number of such rows    s1 = sum 1/2 |v|^2    s2 = sum x_last (the gravity axis)    s3 = sum e(rho)
 *     s4..6 = sum v    s7..9 = sum x cross v    s10..12 = sum x    s13 = max |v|^2    s14, s15 = min, max rho    s16..18, s19..21 = min, max x
 * with e(rho) = ((r^6 - 1)/6 + 1/r) - 1, r = rho/rho0: the compressive energy per unit mass of the Tait equation of state the engine
 * runs (gamma = 7, B = c0^2 rho0 / 7) in units of B/rho0.  Every term is formed in fp64 with one rounding per operation - a host forms
 * the same doubles from a download - and reduced in an order that depends on the particle order alone, on fp32 and fp64 handles alike:
 * repeated runs give the same bits.  Off by default; a handle that never enables it launches what it always did.
 *   enable: after sphmi_upload / sphmi_generate_dam_break_3d, at any later time too.  The handle keeps the newest capacity_steps (>= 1)
 *     samples that have not been read.  A second call drops the series; capacity_steps = 0 disables.  sphmi_upload and the generator
 *     disable.  No step waits for the host: the records of a batch of queued steps come back with the control block the host fetches
 *     anyway.  sphmi_forces_once records nothing.
 *   read: delivers and clears the oldest `capacity` samples recorded since the last read, oldest first: iteration_out / time_out / dt_out
 *     [capacity] as sphmi_group_forces_read; count_out [capacity] n; energy_out [capacity x 3] kinetic m0*s1, potential m0*g*s2 and
 *     compressive m0*(B/rho0)*s3; momentum_out [capacity x 3] m0*s4..6; angular_out [capacity x 3] m0*s7..9, about the origin (2-D
 *     handles: only the third component is non-zero); centre_out [capacity x 3] s10..12 / n, the centre of mass; extremes_out
 *     [capacity x 3] the largest speed sqrt(s13), the smallest and the largest density; box_out [capacity x 6] min x[3], max x[3] (2-D
 *     handles: zero third components) - formed on the host from the raw values, one multiplication or division each; centre, extremes
 *     and box are 0 where n == 0.  Any output pointer may be NULL.  *n_out, *n_dropped, capacity = 0: as sphmi_group_forces_read.
 *   SPHMI_ERR_STATE: before the upload; read while disabled; rank-mode handles (a process holds one slab of the rows).
 *   SPHMI_ERR_ARGUMENT: capacity_steps < 0, negative capacity, null n_out.
 * Multi-device handles of one process: every slab reduces the rows it owns (ghost copies do not count) and the handle combines the
 * slabs' raw records in slab order - sums add, extremes take min or max.  Budgets, probes and group forces may be enabled together.
 */
int sphmi_budgets_enable(sphmi_handle* h, int64_t capacity_steps);
int sphmi_budgets_read(sphmi_handle* h, int64_t capacity, int64_t* iteration_out, double* time_out, double* dt_out,
                       int64_t* count_out, double* energy_out, double* momentum_out, double* angular_out, double* centre_out,
                       double* extremes_out, double* box_out, int64_t* n_out, int64_t* n_dropped);

/*
 * The FLOW through control boxes at STEP resolution, recorded on the device: how much fluid a region holds and how much went in or
 * out - the discharge through a section of a channel, the volume that has passed an obstacle, overtopping of a wall, the filling
 * curve of a compartment.  A box is axis-aligned and half-open: row i is INSIDE box b iff lo[b][d] <= x_i[d] < hi[b][d] for every
 * d < dims, compared in fp64 on the Position doubles sphmi_download would deliver - adjacent boxes partition space without a gap or
 * an overlap.  lo = -inf and hi = +inf are legal: a box unbounded along the other axes is a gate across a channel, and the box
 * [c, +inf) along x counts the crossings of the plane x = c, `entered` in the +x direction, `left` in the -x direction.  Boxes may
 * overlap and may be empty of fluid.  For every executed step and every box, over the rows i of the handle with Type == Fluid, the
 * raw values
 *     s0 = n_after, the rows inside on the state sphmi_download would deliver directly after that step
 *     s1 = sum 1/rho over those rows (one fp64 division per row)    s2..4 = sum v over those rows (2-D handles: an exact zero third)
 *     s5 = entered, the rows NOT inside on the state at the START of that step and inside after it
 *     s6 = left, the rows inside at the start of that step and not inside after it
 * The state at the start of a step is what sphmi_download would have delivered before it, the after-state of the step before: for
 * consecutive samples n_after[k] - n_after[k-1] == entered[k] - left[k] holds exactly, across rebuilds and sphmi_advance calls.  The
 * start state is marked on the device as the first launch of a step (the corrector of an fp32 handle updates positions in place);
 * every crossing between two outputs is counted, one that comes back included.  Sums are reduced in an order that depends on the
 * particle order alone: repeated runs give the same bits.  Off by default; a handle that never enables it launches what it always did.
 *   enable: after sphmi_upload / sphmi_generate_dam_break_3d, at any later time too.  1 <= n_boxes <= SPHMI_MAX_FLOW_BOXES boxes, lo
 *     and hi `dims` doubles per box.  The handle keeps the newest capacity_steps (>= 1) samples that have not been read.  A second
 *     call replaces the boxes and drops the series; n_boxes = 0 disables.  sphmi_upload and the generator disable.  No step waits for
 *     the host: the records of a batch of queued steps come back with the control block the host fetches anyway.  sphmi_forces_once
 *     records nothing.
 *   read: delivers and clears the oldest `capacity` samples recorded since the last read, oldest first: iteration_out / time_out / dt_out
 *     [capacity] as sphmi_group_forces_read; count_out [capacity x n_boxes] n_after; volume_out [capacity x n_boxes] m0*s1;
 *     momentum_out [capacity x n_boxes x 3] m0*s2..4; entered_out, left_out [capacity x n_boxes] - volume and momentum formed on the
 *     host, one multiplication each.  Any output pointer may be NULL.  *n_out, *n_dropped, capacity = 0: as sphmi_group_forces_read.
 *   SPHMI_ERR_STATE: before the upload; read while disabled; rank-mode handles (a process holds one slab of the rows).
 *   SPHMI_ERR_ARGUMENT: a null table, n_boxes out of [0, SPHMI_MAX_FLOW_BOXES], a NaN bound, !(lo < hi) on any axis of any box,
 *     capacity_steps < 1, negative capacity, null n_out.
 * Multi-device handles of one process: every slab marks and samples the rows it owns (ghost copies do not count; rows migrate in the
 * collective rebuild, between steps, so a row's start and end state lie in the same slab) and the handle adds the slabs' records in
 * slab order.  Flow, budgets, probes and group forces may be enabled together.
 */
#define SPHMI_MAX_FLOW_BOXES 16
int sphmi_flow_enable(sphmi_handle* h, int32_t n_boxes, const double* lo, const double* hi, int64_t capacity_steps);
int sphmi_flow_read(sphmi_handle* h, int64_t capacity, int64_t* iteration_out, double* time_out, double* dt_out,
                    int64_t* count_out, double* volume_out, double* momentum_out, int64_t* entered_out, int64_t* left_out,
                    int64_t* n_out, int64_t* n_dropped);

/*
 * ENVELOPES: what every single particle has experienced over time, accumulated on the device at EVERY step - the peak pressure
 * every wall particle of an obstacle has seen, when the wave reached it and the pressure impulse it took (the load MAP of a
 * structure, not only its total), the largest speed every fluid particle ever had.  Such peaks last a few steps and an output
 * interval holds hundreds; without this a caller gets them only by downloading every step.  With, "after a step", the state
 * sphmi_download would deliver directly after that step - P its Pressure, v its Velocity (2-D handles: vz = 0; the device values
 * widened to fp64: a handle with host_float_bytes = 4 on an fp64 device rounds its downloads, the envelopes do not), t =
 * TotalTime at the end of the step, dt its time step - every selected row keeps eight doubles, updated per EXECUTED step:
 *     p_max, t_p_max   start -inf, 0    if (P > p_max) { p_max = P; t_p_max = t; }     strict: the first attainment keeps its time
 *     p_min            start +inf       if (P < p_min) p_min = P
 *     impulse          start 0          impulse = impulse + P * dt
 *     square           start 0          square = square + (P * P) * dt
 *     loaded           start 0          if (P > 0) loaded = loaded + dt
 *     speed2_max       start 0          s = (vx*vx + vy*vy) + vz*vz; if (s > speed2_max) speed2_max = s
 *     t_arrival        start +inf       if (P > 0 && t_arrival == inf) t_arrival = t
 * Every operation is fp64, rounded once, never contracted: a host that downloads after every step forms the same doubles, bit for
 * bit (sphexample_amd/envelopes.py: update).  A NaN never wins a comparison and poisons the sums.  The window is kept with them:
 * steps (executed steps since the enable), t_begin (TotalTime at the enable), t_end, duration = sum dt in step order.  The records
 * follow the PARTICLE, not the row: the sort moves rows at every rebuild, the records stay where they were at the enable and are
 * found through the row column the sorts carry anyway and a map of their own, composed in sphmi_download_permutation as the map of
 * the attached columns is - attaching or detaching columns does not disturb the envelopes, nor the other way round.  No atomics: a
 * record has one writer.  Off by default; a handle that never enables it launches what it always did.
 *   enable: after sphmi_upload / sphmi_generate_dam_break_3d, at any later time too: steps executed before it are not seen.  Bit
 *     Type of type_mask selects the rows of that Type (Fluid = 1, Fixed = 2, Moving = 3, as in sphmi_components_build); rows of
 *     other types keep the start record.  A second call replaces the selection and restarts the window (start records, steps = 0,
 *     t_begin = the TotalTime now); type_mask = 0 disables and frees the memory.  sphmi_upload and the generator disable.  Cancelled
 *     steps add nothing; sphmi_forces_once records nothing.
 *   read: synchronous, between sphmi_advance calls.  *steps_out; window_out[3] = { t_begin, t_end, duration }; then eight arrays of
 *     n = sphmi_owned_count doubles - doubles whatever host_float_bytes is - row i being row i of what sphmi_download delivers
 *     NOW: p_max, t_p_max, p_min, impulse, square, loaded, speed_max = sqrt(speed2_max) (the one sqrt, formed on the host) and
 *     t_arrival (+inf: never loaded).  Any output pointer may be NULL.  It clears nothing: the envelopes keep growing across
 *     sphmi_advance calls, downloads, column downloads, sphmi_download_permutation and the on-demand results.
 *   SPHMI_ERR_STATE: before the upload; read while disabled; rank-mode and multi-device handles (rows migrate between slabs, and
 *     carrying their records along is not built).
 *   SPHMI_ERR_ARGUMENT: a type_mask with a bit other than 1, 2, 3 set (the mask travels as an int32_t - the same register as the
 *     uint32_t of sphmi_components_build - so that the Julia shim's prototype check, which knows no uint32_t, covers the binding; a
 *     negative value has bit 31 set and is refused like any other stray bit).
 *   SPHMI_ERR_DEVICE: the device cannot hold the 68 bytes per row (64 of record, 4 of map; the first sphmi_download_permutation
 *     adds 4 more, a read 8 per requested array); the message gives the bytes, nothing is held and the handle stays usable.
 */
int sphmi_envelopes_enable(sphmi_handle* h, int32_t type_mask);
int sphmi_envelopes_read(sphmi_handle* h, int64_t* steps_out, double* window_out /* [3] t_begin, t_end, duration */,
                         double* p_max_out, double* t_p_max_out, double* p_min_out, double* impulse_out, double* square_out,
                         double* loaded_out, double* speed_max_out, double* t_arrival_out /* each [n] */);

/*
 * MAPS: what every patch of the tank has experienced over time, accumulated on the device at EVERY step - how high the water ever
 * stood over each bin of a lattice, when it first got there, how long the bin stayed wet and the mean flow through it: crest, arrival
 * time, wet duration, time-mean depth and velocity, the flood-map quantities.  The envelopes are the Lagrangian record of a run at
 * step resolution, this is the Eulerian one; sphmi_sample_grid gives such a view at output times only.
 *   The lattice: origin[dims], spacing[dims], counts[dims]; bin (k0, k1[, k2]) has index k0 + counts[0] * (k1 + counts[1] * k2) - the
 *     node order of sphmi_sample_grid - and holds the rows with k_d = floor((x_d - origin_d) / spacing_d), 0 <= k_d < counts_d on
 *     every axis: fp64 on the Position doubles sphmi_download would deliver, one rounding for the subtraction, one for the division,
 *     compared as doubles, so a NaN lies outside.  counts_d = 1 with spacing_d = +inf collapses an axis (every finite coordinate lies
 *     in its one bin): a column map over the floor of a 3-D tank is counts = (nx, ny, 1), spacing = (s, s, +inf).  up_axis names the
 *     coordinate whose extremes are kept.  Only owned Fluid rows count, and of those only rows whose Velocity is finite.
 *   Per executed step and bin: n (the rows inside), top and bottom (max and min of the up_axis coordinate) and S_d = sum of
 *     llrint(v_d * 2^32) per axis (int64, round to nearest even; 2-D handles: an exact zero on the third) - integer adds and max / min
 *     only, which are exactly associative: the result does not depend on the order the device got there, bit for bit.
 *   The record of a bin, twelve doubles, updated only by steps with n > 0; t = TotalTime at the end of the step, dt its time step,
 *     Sd_d = (double)S_d * 2^-32, u_d = Sd_d / (double)n:
 *     top_max, t_top_max       start -inf, 0   if (top > top_max) { top_max = top; t_top_max = t; }
 *     bottom_min               start +inf      if (bottom < bottom_min) bottom_min = bottom
 *     t_arrival                start +inf      if (t_arrival == inf) t_arrival = t
 *     wet                      start 0         wet = wet + dt
 *     fill                     start 0         fill = fill + (double)n * dt
 *     flux[3]                  start 0         flux_d = flux_d + Sd_d * dt
 *     speed2_max, t_speed2_max start 0, 0      s = (ux*ux + uy*uy) + uz*uz; if (s > speed2_max) { speed2_max = s; t_speed2_max = t; }
 *     n_max                    start 0         if ((double)n > n_max) n_max = (double)n
 *     Every operation is fp64, rounded once, never contracted: a host that downloads after every step forms the same doubles, bit for
 *     bit (sphexample_amd/maps.py: update).  The window is kept with them as the envelopes keep theirs.
 *   enable: after sphmi_upload / sphmi_generate_dam_break_3d, at any later time too.  A second call restarts the records (steps = 0,
 *     t_begin = the TotalTime now).  sphmi_maps_disable frees the memory; sphmi_upload and the generator disable.  Cancelled steps add
 *     nothing; sphmi_forces_once records nothing.  Off by default; a handle that never enables it launches what it always did.
 *   read: synchronous, between sphmi_advance calls; clears nothing.  *steps_out; window_out[3] = { t_begin, t_end, duration }; arrays
 *     of bins = product of counts doubles each (flux_out: [bins][3]); speed2_max_out is the SQUARE of the largest bin-mean speed (no
 *     sqrt is taken anywhere).  Then the map of the LAST EXECUTED step, the instantaneous column map: last_n_out [bins], last_top_out
 *     and last_bottom_out [bins] (-inf / +inf in a dry bin), last_velocity_sum_out [bins][3] = Sd.  Any output pointer may be NULL.
 *   SPHMI_ERR_STATE: before the upload; read while disabled; rank-mode and multi-device handles.
 *   SPHMI_ERR_ARGUMENT: a null table, a non-finite origin, a spacing that is NaN or not positive, +inf spacing with a count above 1, a
 *     count below 1, more than SPHMI_MAX_MAP_BINS bins, up_axis outside [0, dims); a handle with more than 2^31 / (4 c0) rows (the
 *     int64 sums S_d cannot overflow while rows * max|v| < 2^31; the message gives the bound).
 *   SPHMI_ERR_DEVICE: the device cannot hold the 184 bytes per bin; nothing is held and the handle stays usable.
 */
#define SPHMI_MAX_MAP_BINS (1 << 20)
int sphmi_maps_enable(sphmi_handle* h, const double* origin, const double* spacing, const int64_t* counts, int32_t up_axis);
int sphmi_maps_disable(sphmi_handle* h);
int sphmi_maps_read(sphmi_handle* h, int64_t* steps_out, double* window_out /* [3] t_begin, t_end, duration */,
                    double* top_max_out, double* t_top_max_out, double* bottom_min_out, double* t_arrival_out, double* wet_out,
                    double* fill_out, double* flux_out /* [bins][3] */, double* speed2_max_out, double* t_speed2_max_out,
                    double* n_max_out, int64_t* last_n_out, double* last_top_out, double* last_bottom_out,
                    double* last_velocity_sum_out /* [bins][3] */);

/*
 * TRACERS: where the water goes, at STEP resolution, recorded on the device - pathlines, residence and transit times, the fate of the
 * water that overtops an obstacle.  Probes sample at fixed points and the envelopes keep the extremes of a row but not its path; a
 * trajectory needed a download after every step.  Two kinds of tracer share one per-step series; either kind may be absent.
 *   TRACKED PARTICLES: up to SPHMI_MAX_TRACERS rows, named in the row order sphmi_download has at the moment of the enable.  After
 *     every executed step each keeps 8 doubles { x[3], v[3], rho, P }: the values sphmi_download would deliver into Float64 host
 *     arrays directly after that step, bit for bit (fp32 handles: record plus low word; P = Pressure!(rho_n+) of the half step; 2-D
 *     handles: a zero third component).  The slots follow the PARTICLE through every sort, found the way the envelopes find their
 *     records, with a map of their own composed in sphmi_download_permutation.  No atomics: a slot has one writer.
 *   DRIFTERS: up to SPHMI_MAX_TRACERS massless points placed anywhere (`dims` doubles each).  Behind every executed step k, with
 *     X the drifter's position before the step and the state after it: the raw sums S, SP, Srho, Sv[3], n of sphmi_probes_enable at X
 *     (the same walk, the same bits a probe at X would record); then
 *         if (S >= min_weight) X[d] = X[d] + (Sv[d] / S) * dt   for d < dims, dt the time step of step k
 *     every operation fp64, rounded once, never contracted (sphexample_amd/tracers.py: step forms the same doubles); otherwise the
 *     drifter is DRY and stays: in empty space, above the surface, outside the particles' bounding grid.  First order in dt, like the
 *     tracer advection of comparable codes.  The record is 10 doubles { X[3] BEFORE the move, S, SP, Srho, Sv[3], n }: a complete
 *     probe sample at a known point.  The move does not depend on the series: samples nobody reads are dropped, the drifter moves on.
 *   enable: after sphmi_upload / sphmi_generate_dam_break_3d, at any later time too.  rows[n_particles], positions[n_drifters x dims],
 *     min_weight finite and positive (0.5: "inside the fluid").  The handle keeps the newest capacity_steps (>= 1) samples that have
 *     not been read.  A second call replaces both sets, drops the series and starts the drifters at the new positions; both counts 0
 *     disables.  sphmi_upload and the generator disable.  Cancelled steps move and record nothing; sphmi_forces_once neither.  Off by
 *     default; a handle that never enables it launches what it always did.
 *   read: delivers and clears the oldest `capacity` samples recorded since the last read, oldest first: iteration_out / time_out /
 *     dt_out [capacity] as sphmi_group_forces_read; particles_out [capacity x n_particles x 8]; drifters_out [capacity x n_drifters x
 *     10]; and, whatever `capacity` is, drifter_positions_out [n_drifters x 3]: X NOW, after the last executed step - the series alone
 *     ends one move short of it.  Any output pointer may be NULL.  *n_out, *n_dropped, capacity = 0: as sphmi_group_forces_read.
 *   SPHMI_ERR_STATE: before the upload; read while disabled; rank-mode and multi-device handles (rows migrate between slabs; neither
 *     their slots nor the drifters are carried along); drifters on handles with H < h.
 *   SPHMI_ERR_ARGUMENT: a count outside [0, SPHMI_MAX_TRACERS], a null table, a row outside [0, n) or named twice, a non-finite
 *     coordinate, a min_weight that is not finite and positive, capacity_steps < 1, negative capacity, null n_out.
 */
#define SPHMI_MAX_TRACERS 1024
int sphmi_tracers_enable(sphmi_handle* h, int32_t n_particles, const int64_t* rows, int32_t n_drifters,
                         const double* positions /* n_drifters x dims */, double min_weight, int64_t capacity_steps);
int sphmi_tracers_read(sphmi_handle* h, int64_t capacity, int64_t* iteration_out, double* time_out, double* dt_out,
                       double* particles_out, double* drifters_out, double* drifter_positions_out, int64_t* n_out, int64_t* n_dropped);

/*
 * MotionDetails of the Geometry with this GroupMarker (src/SimulationGeometry.jl:17-22): particles of Type Moving
 * in that group get Velocity = velocity·direction while start_time <= TotalTime <= start_time + duration (0
 * otherwise) and are displaced by Velocity·dt/2 before each neighbour pass — ProgressMotion,
 * src/SPHCellList.jl:575-596, called at :765 and :787.  `direction` holds `dims` doubles.  At most 16 groups.
 */
int sphmi_set_motion(sphmi_handle* h, uint64_t group_marker, double velocity, double start_time, double duration,
                     const double* direction);

/*
 * One SimulationLoop call (src/SPHCellList.jl:727-805): reset Δx = 1 + h, then step
 * `while TotalTime <= t_target`.  max_steps < 0 means unbounded; otherwise the loop also stops
 * after max_steps steps (used by tests and by the benchmark's fixed-step window).
 */
int sphmi_advance(sphmi_handle* h, double t_target, int64_t max_steps, sphmi_progress* out);

/*
 * Copy particle state back in the engine's current (cell-sorted) order — the same order the
 * reference leaves SimParticles in, because its sort! permutes every field (src/SPHCellList.jl:142).
 * Any pointer may be NULL to skip that field.  cells: N*D Int64 (Particles.Cells).
 */
int sphmi_download(sphmi_handle* h,
                   void* position, void* velocity, void* acceleration,
                   void* density, void* pressure,
                   int64_t* id, uint8_t* type, uint64_t* group_marker,
                   void* ghost_points, int64_t* cells);

/*
 * Parity hook: rebuild the cell list for the current positions, run Pressure! and ONE
 * NeighborLoop!+ReductionStep! (src/SPHCellList.jl:771,774-775) on the current state and return
 * dρdtI (N) and Acceleration (N*D, no gravity) in cell-sorted order; also sorts the particles
 * (as UpdateNeighbors! does) but does not advance time.  apply_mdbc != 0 additionally runs
 * ApplyMDBCBeforeHalf! (:772) between Pressure! and the pair loop.  Multi-device handles: the rebuild is the collective
 * one (migration, fresh ghost layers) and the rows come back merged, in the order one device would hold.
 */
int sphmi_forces_once(sphmi_handle* h, int apply_mdbc, void* drhodt, void* acceleration);

/* Occupied cells in sort order: cells_out receives (index_counter-1)*D Int64 values
 * (UniqueCells[2:IndexCounter], src/SPHCellList.jl:148-157); n_out the count. */
int sphmi_unique_cells(sphmi_handle* h, int64_t* cells_out, int64_t capacity, int64_t* n_out);

/*
 * Per-phase device seconds accumulated since create, under the reference's TimerOutputs labels
 * (src/SPHCellList.jl:748-800).  names_out receives pointers to static strings.  The step phases are timed with
 * HIP events on every 8th step and scaled by 8 (an event pair per phase and step costs more than a small pass);
 * rebuilds are always timed.
 */
int sphmi_timers(sphmi_handle* h, int32_t capacity, const char** names_out, double* seconds_out,
                 int64_t* calls_out, int32_t* n_out);

/* Raw device pointers of the packed neighbour stream (state set A) and the live particle count.  The two packets of a
 * particle are interleaved in ONE array of records: packet h of particle i is pk_h[2*i] (pk1 == pk0 + 1 packet). */
int sphmi_device_ptrs(sphmi_handle* h, void** pk0, void** pk1, int64_t* n_local);

/* ---- measurement hooks (bench.py) ------------------------------------------------------- */
/* Average duration in ms (HIP events on the engine's stream) of the neighbour+force kernel over the
 * launches since the last reset (sampled: the launches of every 8th step), and the number of launches. */
int sphmi_force_kernel_stats(sphmi_handle* h, int reset, double* avg_ms_out, int64_t* launches_out);

/* ---- multi-GPU handles ------------------------------------------------------------------------------------
 * sphmi_create with cfg->n_devices > 1: all slabs in THIS process (what the reference's single Julia process needs).
 * sphmi_create_rank: the same slab driver with ONE slab per process and the other slabs behind RCCL — rank r of `world`
 * processes (torchrun: one process per GPU).  Every process passes the SAME full particle set to sphmi_upload and keeps
 * its slab; sphmi_download then returns the particles this process owns (sphmi_owned_count of them, at most
 * cfg->n_particles).  `unique_id`: the 128 bytes sphmi_rccl_unique_id produced on rank 0, distributed by the launcher
 * (a file, MPI, torch.distributed's store …).  cfg->device is this rank's GPU.
 * SPHMI_TRANSPORT=shm in the environment puts the peers behind a POSIX shared-memory segment of the node instead of
 * RCCL (messages and reductions staged through the host, csrc/sphmi_shm.h): RCCL refuses two ranks on one device, so
 * this is how the rank-mode driver runs — and is tested — with more ranks than GPUs.  Every wait has a deadline
 * (SPHMI_SHM_TIMEOUT seconds, default 120). */
int sphmi_rccl_unique_id(void* id_out /* 128 bytes */);
/* Binds RCCL in this process (dlopen + every symbol the slab driver calls) WITHOUT asking it for an id: ncclGetUniqueId starts a
 * bootstrap root — a listening socket and a thread — per call, so only the rank that hands the id out should call it; the other ranks
 * check with this that their process could join.  SPHMI_ERR_DEVICE + sphmi_last_error(NULL) when RCCL is out of reach. */
int sphmi_rccl_probe(void);
int sphmi_create_rank(const sphmi_config* cfg, int32_t rank, int32_t world, const void* unique_id, sphmi_handle** out);
int sphmi_owned_count(sphmi_handle* h, int64_t* n_out);   /* particles sphmi_download returns (any handle)        */
typedef struct sphmi_multi_info {
    int32_t world, n_local;        /* slabs in total / held by this handle                                         */
    int32_t axis, halo_width;      /* slab axis (0 = x …); ghost-layer width in cell columns (1; 2 + off with mDBC) */
    int32_t transport;             /* 0 = stream-ordered device copies, 1 = RCCL, 2 = host shared memory (below)    */
    int32_t reserved;              /* how the four per-step maxima travel: 0 = the transport's collective (ncclAllReduce), 1 = device mailboxes ($SPHMI_EXCHANGE=mailbox) */
    int64_t n_recuts;              /* rebuilds at which the cuts moved (load balance by work)                        */
    int64_t cuts[SPHMI_MAX_DEVICES];    /* cuts[r-1] = first cell column of slab r                                  */
    int64_t n_live[SPHMI_MAX_DEVICES];  /* particles incl. ghost copies currently held per local slab               */
} sphmi_multi_info;
int sphmi_multi_info_get(sphmi_handle* h, sphmi_multi_info* out);
/* (Test hooks of the slab driver — the shared-memory transport's self-test, initial cuts, host-only planning, the work
 * measure of the re-cut — are declared in include/sphmi_internal.h; they are not part of the drop-in boundary.) */

/*
 * Pressure, density, velocity and fill on a regular lattice, on demand: the sums of sphmi_probes_enable at every node of a lattice,
 * evaluated NOW - a free-surface height map, a slice through an obstacle, a volume of image data - by a kernel that shares the
 * staged particle rows among up to 256 neighbouring nodes (csrc/sphmi_field_grid.h).
 *   Synchronous, called between sphmi_advance calls like sphmi_download; it changes no state a later step, download, column download,
 *   probe series or group-force series reads, and leaves a download begun with sphmi_download_begin alone.
 *   Node (i, j, k) lies at origin[d] + (double)i_d * spacing[d] (one multiply, one add, not fused: a host forms the same doubles); its
 *   index is i + nx * (j + ny * k), x fastest - the order of VTK image data.  `dims` entries of origin, spacing and counts are read.
 *   Per node: n Fluid rows the handle owns within H (inclusive, on the current positions, however stale the cell list), S = sum w_j,
 *   SP, Srho, Sv with w_j = (m0 / rho_j) W(|x_n - x_j|), on the state sphmi_download would deliver now (Pressure = Pressure!(rho_n+) of
 *   the half-step set), all in fp64, no self term, r = 0 legal; summed in row order, without atomics: repeated calls give the same bits.
 *   weight_out [nodes] S, count_out [nodes] n, pressure_out / density_out [nodes] SP / S and Srho / S, velocity_out [nodes x 3] Sv / S
 *   (2-D handles: a zero third component) - normalised on the host, 0 where n == 0; nodes in empty space or outside the cell grid
 *   read zeros.  Any output pointer may be NULL (all NULL: the sums are formed in the device arena and nothing is delivered).
 *   SPHMI_ERR_STATE: before the upload; before the handle has executed its first step since the upload or generator (no cell list, no
 *     half-step set); rank-mode handles; handles with H < h.
 *   SPHMI_ERR_ARGUMENT: null origin, spacing or counts; a non-finite origin; a spacing that is not finite and positive; a count < 1;
 *     more than SPHMI_MAX_GRID_NODES nodes.   SPHMI_ERR_DEVICE: the device cannot hold the result arena (7 doubles per node).
 * Multi-device handles of one process: every slab samples the whole lattice over the rows it owns (ghost copies do not count), the
 * handle adds the slabs' raw sums in slab order and then normalises.
 */
#define SPHMI_MAX_GRID_NODES (1 << 24)
int sphmi_sample_grid(sphmi_handle* h, const double* origin, const double* spacing, const int64_t* counts,
                      double* weight_out, int64_t* count_out, double* pressure_out, double* density_out, double* velocity_out);

/*
 * Pressure, density, velocity and fill at ARBITRARY points, on demand: the sums of sphmi_sample_grid at every point of a cloud that is
 * neither a lattice nor a handful of probes - the panel centroids of a hull, the nodes of another code's mesh, an oblique slice, a ring
 * of sensors - by a kernel that first groups the points by blocks of cells so that up to 256 of them share the staged particle rows
 * (csrc/sphmi_point_cloud.h).  Per point it is the contract of sphmi_sample_grid per node:
 *   Synchronous, called between sphmi_advance calls like sphmi_sample_grid; it changes no state a later step, download, column download,
 *   series read or other on-demand result reads, and leaves a download begun with sphmi_download_begin alone.
 *   positions [n_points x dims], row p the coordinates of point p.  Per point: n Fluid rows the handle owns with
 *   r^2 = ((dx^2 + dy^2) + dz^2) <= H^2 (inclusive, not fused, on the current positions, however stale the cell list), S = sum w_j, SP, Srho,
 *   Sv with w_j = (m0 / rho_j) W(r), on the state sphmi_download would deliver now (Position and Density record + low word on fp32
 *   handles, Pressure = Pressure!(rho_n+) of the half-step set), all in fp64, no self term, r = 0 legal.
 *   weight_out [n_points] S, count_out [n_points] n, pressure_out / density_out [n_points] SP / S and Srho / S, velocity_out
 *   [n_points x 3] Sv / S (2-D handles: a zero third component) - normalised on the host as for the lattice, 0 where n == 0.  Any output
 *   pointer may be NULL.  Outputs are in the CALLER's order: entry p belongs to positions[p].
 *   The result of a point depends on its own coordinates and the state of the handle alone - not on which other points are in the call,
 *   how many there are, or their order: it is summed in ascending row order, without atomics.  A subset of a cloud, the cloud shuffled,
 *   a point given twice in one call and a repeated call all deliver the same bits for that point.
 *   A point in empty space, or outside the particles' cell grid on any side, reads zeros.  n_points == 0 is legal and does nothing.
 *   SPHMI_ERR_STATE: as sphmi_sample_grid - before the upload; before the handle has executed its first step since the upload or
 *     generator; rank-mode handles; handles with H < h.
 *   SPHMI_ERR_ARGUMENT: null positions with n_points > 0; n_points < 0 or above SPHMI_MAX_SAMPLE_POINTS; a coordinate that is not finite
 *     (the text names the index of the first such point).
 *   SPHMI_ERR_DEVICE: the device cannot hold the positions, the plan and the result arena (7 doubles per point; the text names the
 *     bytes of the allocation that failed); the handle stays usable.
 * Multi-device handles of one process: every slab samples all points over the rows it owns (ghost copies do not count), the handle adds
 * the slabs' raw sums in slab order and then normalises.
 */
#define SPHMI_MAX_SAMPLE_POINTS (1 << 24)
int sphmi_sample_points(sphmi_handle* h, int64_t n_points, const double* positions /* n_points x dims */,
                        double* weight_out, int64_t* count_out, double* pressure_out, double* density_out, double* velocity_out);

/*
 * The GRADIENTS of pressure, density, velocity and fill at arbitrary points, on demand: a vorticity slice through a breaking wave, the
 * strain rate on the panels of a hull, the pressure gradient along a wall, the free-surface normal at the nodes of another code's mesh -
 * without a download and a neighbour search on the host (csrc/sphmi_point_gradients.h; the cloud is binned as for sphmi_sample_points).
 * Calling convention, limits, state and errors are those of sphmi_sample_points; what differs is what comes back.  Per point x, over the
 * Fluid rows j the handle owns with r^2 = ((dx^2 + dy^2) + dz^2) <= H^2 (the cut of sphmi_sample_points), V_j = m0 / rho_j, W and W' the
 * handle's kernel, g_j = W'(r) (x - x_j) / r, on the state sphmi_download would deliver now, all in fp64, no self term; a row at r = 0
 * counts in n and the S sums and adds nothing to the G sums:
 *   weight_out        [n_points]          S        = sum V_j W
 *   count_out         [n_points]          n        = rows that pass the cut
 *   sum_pressure_out  [n_points]          SP       = sum V_j P_j W
 *   sum_density_out   [n_points]          Srho     = sum V_j rho_j W
 *   sum_velocity_out  [n_points x 3]      Sv[a]    = sum V_j v_j[a] W
 *   grad_weight_out   [n_points x 3]      G[b]     = sum V_j g_j[b]
 *   grad_pressure_out [n_points x 3]      GP[b]    = sum V_j P_j g_j[b]
 *   grad_density_out  [n_points x 3]      Grho[b]  = sum V_j rho_j g_j[b]
 *   grad_velocity_out [n_points x 3 x 3]  Gv[a][b] = sum V_j v_j[a] g_j[b]      (entry 9 p + 3 a + b)
 * Every sum is delivered RAW - nothing is divided by S here, unlike sphmi_sample_points: S, n, SP, Srho and Sv are the raw sums behind that
 * call's outputs, bit for bit.  The caller normalises; the Shepard-corrected difference form grad A ~ (GA - (SA / S) G) / S is exact for a
 * constant field whatever the particle disorder (sphexample_amd/fields.py: velocity_gradient, vorticity_at, divergence_at, strain_rate,
 * pressure_gradient, surface_normal_at).  2-D handles write exact zeros to every z slot.  Any output pointer may be NULL.  Outputs are in
 * the CALLER's order, and a point's result depends on its own coordinates and the state of the handle alone: rows are added in ascending
 * row order, without atomics.  A point in empty space or outside the particles' cell grid reads zeros; n_points == 0 is legal.
 *   SPHMI_ERR_STATE, SPHMI_ERR_ARGUMENT, SPHMI_ERR_DEVICE: as sphmi_sample_points (the arena holds 25 doubles per point).
 * Multi-device handles of one process: every sum is linear in the rows, so every slab samples all points over the rows it owns and the
 * handle adds the slabs' raw sums in slab order.  (sphmi_particle_fields, the same quantities AT the particles, stays single-device.)
 */
int sphmi_sample_point_gradients(sphmi_handle* h, int64_t n_points, const double* positions /* n_points x dims */,
                                 double* weight_out, int64_t* count_out, double* sum_pressure_out, double* sum_density_out,
                                 double* sum_velocity_out, double* grad_weight_out, double* grad_pressure_out, double* grad_density_out,
                                 double* grad_velocity_out);

/*
 * The MOMENTS of the kernel weights at arbitrary points, on demand: what a linear (first-order moving-least-squares) fit of pressure,
 * density and velocity AT a point needs - a pressure sensor on a wall or on the bed, a probe within H of the free surface, wherever the
 * support is one-sided and the Shepard mean of sphmi_sample_points reads the field at the centroid of the neighbours instead of at the
 * point (csrc/sphmi_point_moments.h; the cloud is binned as for sphmi_sample_points).  Calling convention, limits, state and errors are
 * those of sphmi_sample_points; what differs is what comes back.  Per point x, over the Fluid rows j the handle owns with
 * r^2 = ((dx^2 + dy^2) + dz^2) <= H^2 (the cut of sphmi_sample_points: inclusive, not fused, on the current positions),
 * w_j = (m0 / rho_j) W(r), e_j = x_j - x, on the state sphmi_download would deliver now, all in fp64, no self term; a row at r = 0
 * counts in n and the zeroth sums and adds nothing to the others:
 *   weight_out          [n_points]          S        = sum w
 *   count_out           [n_points]          n        = rows that pass the cut
 *   sum_pressure_out    [n_points]          SP       = sum w P
 *   sum_density_out     [n_points]          Srho     = sum w rho
 *   sum_velocity_out    [n_points x 3]      Sv[a]    = sum w v[a]
 *   moment1_out         [n_points x 3]      M1[b]    = sum w e[b]
 *   moment2_out         [n_points x 6]      M2[bc]   = sum w e[b] e[c]      (xx, xy, xz, yy, yz, zz)
 *   moment_pressure_out [n_points x 3]      P1[b]    = sum w P e[b]
 *   moment_density_out  [n_points x 3]      R1[b]    = sum w rho e[b]
 *   moment_velocity_out [n_points x 3 x 3]  V1[a][b] = sum w v[a] e[b]      (entry 9 p + 3 a + b)
 * Every sum is delivered RAW: S, n, SP, Srho and Sv are the sums sphmi_sample_point_gradients delivers, bit for bit.  The caller solves
 * [[S, M1^T], [M1, M2]] [a; b] = [sum w f; sum w f e] per point and field: a is the field AT the point, b its gradient, exact for a
 * linear field whatever the particle disorder and however one-sided the support (sphexample_amd/fields.py: linear_fit, which falls back
 * to the Shepard mean where the support cannot carry a plane).  2-D handles write exact zeros to every slot of the third axis.  Any
 * output pointer may be NULL.  Outputs are in the CALLER's order, and a point's result depends on its own coordinates and the state of
 * the handle alone: rows are added in ascending row order, without atomics.  A point in empty space or outside the particles' cell
 * grid reads zeros; n_points == 0 is legal.
 *   SPHMI_ERR_STATE, SPHMI_ERR_ARGUMENT, SPHMI_ERR_DEVICE: as sphmi_sample_points (the arena holds 31 doubles per point).
 * Multi-device handles of one process: every sum is linear in the rows, so every slab samples all points over the rows it owns and the
 * handle adds the slabs' raw sums in slab order.
 */
int sphmi_sample_point_moments(sphmi_handle* h, int64_t n_points, const double* positions /* n_points x dims */,
                               double* weight_out, int64_t* count_out, double* sum_pressure_out, double* sum_density_out,
                               double* sum_velocity_out, double* moment1_out, double* moment2_out, double* moment_pressure_out,
                               double* moment_density_out, double* moment_velocity_out);

/*
 * WHERE ALONG A LINE DOES THE WATER BEGIN, on demand: the first crossing of S = level along rays - the water level at a gauge, the run-up
 * along a slope, the wetted height on an obstacle, the depth image a viewer renders from - found on the device by a march and a
 * subdivision instead of columns of fixed probes, a sample of every point of every line or a whole lattice (csrc/sphmi_rays.h).
 *   Synchronous, called between sphmi_advance calls like sphmi_sample_points; it changes no state a later step, download, column
 *   download, series read or other on-demand result reads, and leaves a download begun with sphmi_download_begin alone.
 *   Ray r: origins / directions [n_rays x dims], t_begin / t_end [n_rays].  At the parameter t the point is x[a] = o[a] + t d[a], one
 *   multiply then one add, not fused; d need not be a unit vector, t and step are in units of |d|.  At x the sums are those of
 *   sphmi_sample_point_gradients, bit for bit: n, S, SP, Srho, Sv over the Fluid rows the handle owns with
 *   r^2 = ((dx^2 + dy^2) + dz^2) <= H^2 on the state sphmi_download would deliver now, fp64, ascending row order, no self term.
 *   inside(t) is S(t) >= level; a point outside the particles' cell grid reads zeros and is outside.
 *   March: K = (int64) ceil((t_end - t_begin) / step) in fp64; t_k = t_begin + (double)k step for k < K, t_K = t_end exactly.  The
 *   crossing is the smallest k in 1 .. K at which the two ends of the interval disagree the way `mode` asks - SPHMI_RAY_ENTER:
 *   !inside(t_(k-1)) && inside(t_k); SPHMI_RAY_LEAVE: the reverse; SPHMI_RAY_ANY: either.
 *   Refinement: from (a, b) = (t_(k-1), t_k), SPHMI_RAY_REFINE_ROUNDS rounds of: delta = (b - a) * 0.015625; u_m = a + (double)m delta
 *   for m = 1 .. 63, u_0 = a, u_64 = b; the new bracket is (u_(m-1), u_m) for the smallest m in 1 .. 64 whose side differs from the side
 *   of a.  A round with delta == 0 leaves the bracket as it is.  Four rounds narrow the interval by 2^24.
 *   status_out   [n_rays]      bit 0: a crossing was found; bit 1: inside(t_0)
 *   interval_out [n_rays]      k, or -1
 *   bracket_out  [n_rays x 2]  the final (a, b)
 *   point_out    [n_rays x 3]  x at the INSIDE end of the bracket - b for an entering crossing, a for a leaving one - and there
 *   weight_out, count_out, sum_pressure_out, sum_density_out [n_rays], sum_velocity_out [n_rays x 3]: S, n, SP, Srho, Sv, RAW as
 *   sphmi_sample_point_gradients delivers them at point_out; the record always describes fluid, S >= level.
 *   A ray without a crossing delivers NaN brackets and points and zero sums.  2-D handles write exact zeros to every z slot.  Any output
 *   pointer may be NULL.  Outputs are in the CALLER's order, and a ray's result depends on its own arguments and the state of the handle
 *   alone.  n_rays == 0 is legal; t_end == t_begin is legal and finds no crossing.  A hit behind the first is the caller's: cast again
 *   from bracket[1].
 *   SPHMI_ERR_STATE: as sphmi_particle_fields - before the upload; before the first executed step since the upload or generator; handles
 *     with H < h; rank-mode handles; multi-device handles (a crossing needs the slabs' COMBINED S at every evaluation of the search,
 *     which is not built).
 *   SPHMI_ERR_ARGUMENT: null origins, directions, t_begin or t_end with n_rays > 0; n_rays < 0 or above SPHMI_MAX_RAYS; a coordinate or
 *     parameter that is not finite (the text names the first such ray); a zero direction; t_end < t_begin; step or level not finite
 *     or <= 0; K above SPHMI_MAX_RAY_POINTS; an unknown mode.
 *   SPHMI_ERR_DEVICE: the device cannot hold the arena (2 dims + 15 words of 8 bytes and 2 of 4 per ray); the handle stays usable.
 */
#define SPHMI_MAX_RAYS            (1 << 20)
#define SPHMI_MAX_RAY_POINTS      (1 << 16)     /* march intervals per ray */
#define SPHMI_RAY_REFINE_ROUNDS   4
enum { SPHMI_RAY_ENTER = 0, SPHMI_RAY_LEAVE = 1, SPHMI_RAY_ANY = 2 };
int sphmi_cast_rays(sphmi_handle* h, int64_t n_rays,
                    const double* origins /* n x dims */, const double* directions /* n x dims */,
                    const double* t_begin /* n */, const double* t_end /* n */,
                    double step, double level, int32_t mode,
                    int32_t* status_out /* n */, int64_t* interval_out /* n */, double* bracket_out /* n x 2 */,
                    double* point_out /* n x 3 */, double* weight_out, int64_t* count_out,
                    double* sum_pressure_out, double* sum_density_out, double* sum_velocity_out /* n x 3 */);

/*
 * Differential fields AT THE PARTICLES, on demand: vorticity, velocity divergence, the free-surface indicator div r, the free-surface
 * normal, the Shepard sum and the neighbour count of every row - what a post-processor colours a breaking wave by or extracts a free
 * surface from - by a kernel that shares the staged rows among 256 consecutive target rows (csrc/sphmi_particle_fields.h).
 *   Synchronous, called between sphmi_advance calls like sphmi_sample_grid; it changes no state a later step, download, column download,
 *   probe series, group-force series or sphmi_sample_grid reads, and leaves a download begun with sphmi_download_begin alone.
 *   n = sphmi_owned_count rows; row i of every output is row i of what sphmi_download delivers now.  Outputs are doubles whatever
 *   host_float_bytes is.  Any output pointer may be NULL (all NULL: the sums are formed in the device arena and nothing is delivered).
 *   For every row i, of any Type, over every row j != i of any Type with r^2 = |x_i - x_j|^2 <= H^2 (inclusive, on the current positions,
 *   however stale the cell list; r^2 = ((dx^2 + dy^2) + dz^2), not fused), with V_j = m0 / rho_j, W the handle's kernel and
 *   grad_i W_ij = W'(r) (x_i - x_j) / r, on the Position, Velocity and Density sphmi_download would deliver now (no pressure is involved):
 *     count_out      n_i       the number of such j
 *     shepard_out    S_i       V_i W(0) + sum V_j W_ij            (the self term is in: i is a particle; about 1 inside the fluid)
 *     normal_out     N_i       sum V_j grad_i W_ij                (about 0 inside; the gradient of the colour function: at a free surface
 *                                                                 it points INTO the fluid, the outward normal is -N / |N|)
 *     div_r_out      (div r)_i sum V_j (x_j - x_i) . grad_i W_ij  (about dims inside; lower at a free surface)
 *     div_v_out      (div v)_i sum V_j (v_j - v_i) . grad_i W_ij
 *     vorticity_out  w_i       sum V_j grad_i W_ij x (v_j - v_i)  (a rigid rotation v = Omega x x gives 2 Omega)
 *   2-D handles deliver only the z component of the vorticity: its x and y, and the third component of N, are exact zeros.  A coincident
 *   row (r = 0) counts in n and S and adds nothing to the four gradient sums.  All in fp64, summed in row order without atomics:
 *   repeated calls give the same bits.
 *   SPHMI_ERR_STATE: before the upload; before the handle has executed its first step since the upload or generator (no cell list);
 *     handles with H < h; rank-mode handles; multi-device handles - after the corrector a slab's ghost copies hold the half-step state,
 *     so a slab cannot see its neighbours' current rows without a halo exchange of its own, which is not built.
 *   SPHMI_ERR_DEVICE: the device cannot hold the result arena (10 doubles per row).
 */
int sphmi_particle_fields(sphmi_handle* h,
        int64_t* count_out,      /* [n]      n_i       */
        double*  shepard_out,    /* [n]      S_i       */
        double*  normal_out,     /* [n x 3]  N_i       */
        double*  div_r_out,      /* [n]      div r     */
        double*  div_v_out,      /* [n]      div v     */
        double*  vorticity_out); /* [n x 3]  w_i       */

/*
 * The neighbour list of every row in CSR form, built on the device on demand: who the neighbours ARE, for the pair sums the library does
 * not define - a user viscosity or diffusion term, a pair statistic - formed on the host from the list and one download, without a
 * neighbour search there (csrc/sphmi_neighbor_list.h).
 *   sphmi_neighbors_build is synchronous and called between sphmi_advance calls like sphmi_particle_fields; it changes no state a later
 *   step, download, column download, series read, sphmi_sample_grid or sphmi_particle_fields reads, and leaves a download begun with
 *   sphmi_download_begin alone.  n_rows = sphmi_owned_count rows; row i is row i of what sphmi_download delivers now.
 *   Row i, of any Type, lists every row j != i of any Type with r^2 = ((dx^2 + dy^2) + dz^2) <= H^2 - inclusive, not fused, on the
 *   Position doubles sphmi_download would deliver now (fp32 handles: record + low word), however stale the cell list: the cut of
 *   sphmi_particle_fields, which a host reproduces bit for bit; its count_out is the length of every row.  Coincident rows are listed;
 *   j = i is excluded by row index.  SPHMI_NEIGHBORS_FULL lists both (i, j) and (j, i); SPHMI_NEIGHBORS_HALF keeps j > i, every pair once.
 *   The list of a row is strictly ascending in j and no atomics decide an entry's place: repeated calls give the same bytes.
 *   The entries of row i are neighbors[offsets[i] .. offsets[i + 1]), 0-based, offsets[0] = 0, offsets[n_rows] = n_pairs.  Offsets are
 *   int64 and the scan that forms them sums in 64 bits: at the per-device particle limit the total passes 2^31.  (That is reviewed, not
 *   exercised: offsets beyond 2^31 need more than 10^7 rows.)
 *   The result stays in a device arena of the handle until the next build, sphmi_neighbors_release (which gives the memory back) or
 *   sphmi_destroy.  sphmi_advance, sphmi_upload, sphmi_generate_dam_break_3d and sphmi_forces_once mark it stale: rows may have moved.
 *   sphmi_neighbors_read copies the offsets [n_rows + 1] and the entries [n_pairs] to host arrays; either pointer may be NULL.
 *   SPHMI_ERR_STATE: before the upload; before the handle has executed its first step since the upload or generator (no cell list);
 *     handles with H < h; rank-mode handles; multi-device handles (single-device handles only, as for sphmi_particle_fields);
 *     sphmi_neighbors_read without a build, or of a stale result.
 *   SPHMI_ERR_ARGUMENT: an unknown mode; a null n_pairs_out (n_rows_out may be NULL).
 *   SPHMI_ERR_DEVICE: the device cannot hold the arena (4 bytes per entry); the message gives the pair count and the bytes, and the
 *     handle stays usable.
 */
enum { SPHMI_NEIGHBORS_FULL = 0, SPHMI_NEIGHBORS_HALF = 1 };
int sphmi_neighbors_build(sphmi_handle* h, int32_t mode, int64_t* n_rows_out, int64_t* n_pairs_out);
int sphmi_neighbors_read(sphmi_handle* h, int64_t* offsets_out /* [n_rows + 1] */, int32_t* neighbors_out /* [n_pairs] */);
int sphmi_neighbors_release(sphmi_handle* h);

/*
 * The free surface as GEOMETRY, extracted on the device on demand: the surface S = level of the Shepard sum of sphmi_sample_grid's
 * lattice - about 1 in the fluid, 1/2 at the surface, 0 in air - as a triangle mesh (3-D handles) or a contour polyline (2-D handles):
 * an overturning wave, a splash, a cavity behind an obstacle, which a height map cannot hold (csrc/sphmi_isosurface.h,
 * csrc/sphmi_iso_core.h).  Only the mesh crosses the bus; nothing of S does.
 *   sphmi_isosurface_build is synchronous and called between sphmi_advance calls like sphmi_sample_grid, with the same lattice
 *   arguments; it changes no state a later step, download, column download, series read, sphmi_sample_grid, sphmi_particle_fields or
 *   neighbour list reads, and leaves a download begun with sphmi_download_begin alone.
 *   Node n is INSIDE iff S[n] >= level.  Every cell - named by its lowest node, x fastest - is cut into D! Kuhn simplices along its main
 *   diagonal: for an axis permutation p, w_0 = the lowest corner, w_k = w_(k-1) + e_p(k); neighbouring cells agree on every face
 *   diagonal, so the surface is watertight by construction.  A lattice with a count of 1 along an axis has no cells: an empty mesh.
 *   Edges: node a to b = a + m, m in 1 .. 2^D - 1 a bitmask of unit steps (bit d: a step along axis d); a owns the edge in slot m - 1;
 *   it exists if b is on the lattice and crosses iff exactly one end is inside.
 *   Vertices: one per crossing edge, at x_a + t (x_b - x_a) with t = (level - S_a) / (S_b - S_a), always from the owner a, the node
 *   coordinates formed as sphmi_sample_grid forms them, every operation in fp64 and rounded once (not fused): a host forms the same
 *   doubles.  Order: owner ascending, then slot ascending.  vertices_out is [n_vertices x 3]; 2-D handles: an exact zero third component.
 *   Elements: int32 triples (3-D) or pairs (2-D) of vertex indices; cell ascending, within a cell the simplices in the lexicographic
 *   order of p, within a simplex (corners named by their position 0 .. D in w):
 *     3-D, one corner inside or one corner outside: that corner a; the triangle of the edges (a, b), b != a ascending.
 *     3-D, two inside a < b, two outside c < d: the triangles [(a,c), (a,d), (b,d)] and then [(a,c), (b,d), (b,c)].
 *     In every 3-D case the first vertex stays and the other two are swapped where needed so that the normal (v1 - v0) x (v2 - v0)
 *     points from the inside corners to the outside ones, out of the fluid.
 *     2-D: the segment between the two crossing edges, directed so that the inside lies to its left.
 *   Degenerate elements (t = 0: a node exactly at the level) are legal and kept.  No hash table and no atomics place a vertex or an
 *   element: repeated calls give the same bytes.
 *   Attributes: pressure_out [n_vertices] and velocity_out [n_vertices x 3] are A_a + t (A_b - A_a), the same t, not fused, of the means
 *   SP / S and Sv / S sphmi_sample_grid delivers (one division each, 0 where n == 0); if exactly one end has n == 0 the other end's
 *   mean is taken unmixed.  They are always formed at the build (4 doubles per vertex); the read delivers what is asked for.
 *   The result stays in a device arena of its own until the next build, sphmi_isosurface_release (which gives the memory back) or
 *   sphmi_destroy; a later sphmi_sample_grid does not touch it.  sphmi_advance, sphmi_upload, sphmi_generate_dam_break_3d and
 *   sphmi_forces_once mark it stale: rows may have moved.  sphmi_isosurface_read copies the mesh to host arrays; any pointer may be NULL.
 *   SPHMI_ERR_STATE: before the upload; before the handle has executed its first step since the upload or generator (no cell list, no
 *     half-step set); handles with H < h; rank-mode handles; multi-device handles (single-device handles only: a multi-device handle
 *     adds the slabs' lattice sums on the host, no device holds S); sphmi_isosurface_read without a build, or of a stale or released
 *     result.
 *   SPHMI_ERR_ARGUMENT: everything sphmi_sample_grid reports of a lattice; a level that is not finite and positive; a null
 *     n_vertices_out or n_elements_out.
 *   SPHMI_ERR_DEVICE: the device cannot hold the arena (25 bytes per node, 56 per vertex, 4 D per element); the message gives the
 *     counts and the bytes, and the handle stays usable.
 */
int sphmi_isosurface_build(sphmi_handle* h, const double* origin, const double* spacing, const int64_t* counts,
                           double level, int64_t* n_vertices_out, int64_t* n_elements_out);
int sphmi_isosurface_read(sphmi_handle* h, double* vertices_out /* [nv x 3] */, int32_t* elements_out /* [ne x dims] */,
                          double* pressure_out /* [nv] */, double* velocity_out /* [nv x 3] */);
int sphmi_isosurface_release(sphmi_handle* h);

/*
 * The connected bodies of the fluid, labelled on the device on demand: which rows still belong to the main body of water and which are
 * spray - droplet count, size distribution, the mass detached from the bulk - without a connected-components search on the host
 * (csrc/sphmi_components.h).
 *   sphmi_components_build is synchronous and called between sphmi_advance calls like sphmi_neighbors_build; it changes no state a later
 *   step, download, column download, series read, sphmi_sample_grid, sphmi_particle_fields, neighbour list or mesh reads, and leaves a
 *   download begun with sphmi_download_begin alone.  n_rows = sphmi_owned_count rows; row i is row i of what sphmi_download delivers now.
 *   Rows: a row is SELECTED iff bit Type of type_mask is set - Fluid = 1, Fixed = 2, Moving = 3: 1u << 1 selects the fluid.
 *   Edges: two selected rows i != j are linked iff r^2 = ((dx^2 + dy^2) + dz^2) <= link * link, the product formed once on the host in
 *   fp64; r^2 exactly as the neighbour list forms it - on the Position doubles sphmi_download would deliver now (fp32 handles: record +
 *   low word), term by term, not fused, inclusive, however stale the cell list.  Coincident rows are linked.
 *   Components: a component is a connected set of selected rows; its FIRST ROW is its smallest row index; components are numbered
 *   0 .. C - 1 in ascending first row.
 *   Outputs: label_out[i] is the component number of row i, or -1 if row i is not selected; first_row_out[c] the component's first row;
 *   count_out[c] its number of rows; box_out[c] = { min x, min y, min z, max x, max y, max z } of those Position doubles (2-D handles:
 *   the z entries are exact zeros).  Every output is a function of the state alone: the union-find's compare-and-swap decides the shape
 *   of a forest, never a value, the table is formed with integer add / min / max; repeated builds give the same bytes.
 *   Any pointer of sphmi_components_read may be NULL.
 *   The result stays in a device arena of its own until the next build, sphmi_components_release (which gives the memory back) or
 *   sphmi_destroy.  sphmi_advance, sphmi_upload, sphmi_generate_dam_break_3d and sphmi_forces_once mark it stale: rows may have moved.
 *   SPHMI_ERR_STATE: before the upload; before the handle has executed its first step since the upload or generator (no cell list);
 *     handles with H < h; rank-mode handles; multi-device handles (single-device handles only, as for the neighbour list);
 *     sphmi_components_read without a build, or of a stale or released result.
 *   SPHMI_ERR_ARGUMENT: a link that is not finite, not positive or greater than H (the walk reaches no further); a type_mask with none
 *     of the bits 1 - 3 set, or with any other bit set; a null n_components_out (n_rows_out may be NULL).
 *   SPHMI_ERR_DEVICE: the device cannot hold the arena (24 bytes per row, 56 per component) - the handle stays usable; or the
 *     union-find left the bounds every one of its loops carries (a defect, reported instead of a hung device).
 */
int sphmi_components_build(sphmi_handle* h, double link, uint32_t type_mask,
                           int64_t* n_rows_out, int64_t* n_components_out);
int sphmi_components_read(sphmi_handle* h, int32_t* label_out /* [n_rows] */, int32_t* first_row_out /* [C] */,
                          int32_t* count_out /* [C] */, double* box_out /* [C x 6] */);
int sphmi_components_release(sphmi_handle* h);

/*
 * A selected subset of the rows, compacted on the device on demand: the slice a viewer draws, the Fluid rows, every 8th particle of a
 * movie, the rows a mask flagged, the rows with P above a level - only those cross the bus, in the layout of sphmi_download, instead
 * of every row followed by a mask on the host (csrc/sphmi_select.h).
 *   sphmi_select_build is synchronous and called between sphmi_advance calls; it needs an upload and nothing more - no cell list, no
 *   first step.  It changes no state a later step, download, column download, series read or on-demand result reads, and leaves a
 *   download begun with sphmi_download_begin alone: it stages in buffers of its own, not in those of the pending snapshot.
 *   n_rows = sphmi_owned_count rows; row i is row i of what sphmi_download delivers now.
 *   Selection rule: a row is selected iff EVERY enabled clause holds - the clauses are ANDed; the boxes inside the spatial clause are ORed.
 *     type_mask  bit (Type - 1) is set: 1 Fluid, 2 Fixed, 4 Moving; always on, 7 keeps every row.
 *     boxes      n_boxes > 0: for SOME box b, box_lo[b][d] <= x[d] < box_hi[b][d] for every d < dims (n_boxes x dims doubles each, the
 *                half-open test of sphmi_flow_enable; -inf / +inf allowed; a box with lo >= hi on an axis holds nothing).
 *     markers    n_markers > 0: GroupMarker is one of markers[].
 *     id         id_stride > 1: (uint64)ID % id_stride == id_phase.  Keyed on ID, not on the row: a decimated movie follows the same
 *                particles through every sort.
 *     field      field != SPHMI_SELECT_FIELD_NONE: field_lo <= value <= field_hi, both ends inclusive; a NaN value is never kept.
 *     row_mask   not NULL: n_rows bytes in the CURRENT row order, a non-zero byte keeps the row (copied at the build).
 *   Values the clauses read: the doubles a handle with Float64 host arrays would deliver for that row at this moment - Position is
 *   record + low word on fp32 handles; Density has its sign stripped (and its low word added); Pressure is Pressure!(rho_n+) of the last
 *   step's half-step set, or before the first step the value the upload left, the branch sphmi_download takes;
 *   SPEED2 = (vx * vx + vy * vy) + vz * vz of the Velocity doubles (2-D handles: vz = 0), one rounding per operation, never contracted.
 *   The host float type and sphmi_set_output_components change what is DELIVERED, never what is SELECTED: a host reproduces the selection
 *   bit for bit from a Float64 download (sphexample_amd/selection.py: restate).
 *   Row order: the selected rows come back ascending.  A flag per row, an exclusive scan and rows[offsets[i]] = i: no atomic decides a
 *   place, repeated builds give the same bytes.
 *   The result stays in a device arena of the handle until the next build, sphmi_select_release (which gives the memory back) or
 *   sphmi_destroy.  sphmi_advance, sphmi_upload, sphmi_generate_dam_break_3d and sphmi_forces_once mark it stale: rows may have moved.
 *   sphmi_select_read copies the n_selected row numbers, ascending, 0-based, to rows_out (NULL: nothing is copied).
 *   sphmi_select_download has the signature and the per-field meaning of sphmi_download with n_selected rows per array, slot s holding
 *   row rows[s]: a NULL pointer skips that field, floats in the host float type, vectors padded to 3 components after
 *   sphmi_set_output_components(h, 3) as sphmi_download pads them, cells always n_selected x dims.  Every array equals the rows rows[]
 *   of what sphmi_download delivers now, byte for byte.  sphmi_select_download_columns delivers the attached columns
 *   (sphmi_attach_columns) for the same rows, n_selected x row_bytes[c] each; a NULL entry skips a column.  Both are synchronous -
 *   a selection is small by construction; there is no begin / end pair.
 *   SPHMI_ERR_ARGUMENT: a null sel or a null n_selected_out (n_rows_out may be NULL); a type_mask of 0 or above 7; n_boxes or n_markers
 *     negative or above its maximum, or positive with a null table; id_stride < 1 or id_phase outside [0, id_stride); an unknown field;
 *     a NaN box bound, or a NaN field bound with a field clause; a null table of sphmi_select_download_columns.
 *   SPHMI_ERR_STATE: before the upload; rank-mode handles; multi-device handles (single-device handles only, as for the neighbour list);
 *     sphmi_select_read / _download / _download_columns without a build, or of a stale or released result;
 *     sphmi_select_download_columns with nothing attached.
 *   SPHMI_ERR_DEVICE: the device cannot hold the arena (17 bytes per row: flag, row, offset, mask) or the staging of a download; the
 *     message gives the bytes, and the handle stays usable.
 */
enum { SPHMI_SELECT_FIELD_NONE = 0, SPHMI_SELECT_FIELD_DENSITY, SPHMI_SELECT_FIELD_PRESSURE, SPHMI_SELECT_FIELD_SPEED2 };
#define SPHMI_MAX_SELECT_BOXES   16
#define SPHMI_MAX_SELECT_MARKERS 16
typedef struct sphmi_selection {
    uint32_t        type_mask;            /* bit (Type-1): 1 Fluid, 2 Fixed, 4 Moving; 1..7                        */
    int32_t         n_boxes;              /* 0 = no spatial clause; else the UNION of the boxes                    */
    const double*   box_lo;               /* n_boxes x dims, lo <= x < hi per axis, +-inf allowed (sphmi_flow's test) */
    const double*   box_hi;
    int32_t         n_markers;            /* 0 = no clause; else GroupMarker is one of markers[]                   */
    const uint64_t* markers;
    int64_t         id_stride, id_phase;  /* keep (uint64)ID % id_stride == id_phase; stride 1 = no clause          */
    int32_t         field;                /* SPHMI_SELECT_FIELD_*                                                  */
    double          field_lo, field_hi;   /* keep field_lo <= value <= field_hi; a NaN value is never kept          */
    const uint8_t*  row_mask;             /* NULL, or n_rows bytes in the CURRENT row order; non-zero keeps         */
} sphmi_selection;

int sphmi_select_build(sphmi_handle* h, const sphmi_selection* sel, int64_t* n_rows_out, int64_t* n_selected_out);
int sphmi_select_read(sphmi_handle* h, int32_t* rows_out /* [n_selected], ascending */);
int sphmi_select_download(sphmi_handle* h, void* position, void* velocity, void* acceleration, void* density, void* pressure,
                          int64_t* id, uint8_t* type, uint64_t* group_marker, void* ghost_points, int64_t* cells);
int sphmi_select_download_columns(sphmi_handle* h, void* const* columns_out);
int sphmi_select_release(sphmi_handle* h);

/*
 * The MOMENT sums at fixed PROBE points at STEP resolution, recorded on the device: the sums of sphmi_sample_point_moments behind every
 * executed step, as sphmi_probes_enable records its Shepard sums - a pressure sensor on a wall or on the bed whose signal is FITTED at
 * the sensor (sphexample_amd/fields.py: linear_fit; sphexample_amd/probes.py: fit_series over a whole series), exact for a linear field
 * however one-sided the support, without stopping sphmi_advance for an on-demand call per step (csrc/sphmi_probe_moments.h).
 * An observer of its own with its own point set: independent of sphmi_probes_enable, both may be on together, with each other and with
 * every other observer.  The contract is that of sphmi_probes_enable / sphmi_probes_read wherever it applies:
 *   enable: after sphmi_upload / sphmi_generate_dam_break_3d, at any later time too.  1 <= n_probes <= SPHMI_MAX_PROBES finite points,
 *     positions[n_probes x dims]; a probe in empty space or outside the particles' bounding grid is legal and yields zeros.  The handle
 *     keeps the newest capacity_steps (>= 1) samples that have not been read.  A second call replaces the set and drops the series;
 *     n_probes = 0 disables.  sphmi_upload and the generator disable.  No step waits for the host: the records of a batch of queued
 *     steps come back with the control block the host fetches anyway.  sphmi_forces_once records nothing.  Off by default; a handle that
 *     never enables it launches what it always did.
 *   Per executed step and probe p at x_p, over the Fluid rows j the handle owns with r^2 = ((dx^2 + dy^2) + dz^2) <= H^2 (inclusive, not
 *     fused) on the state sphmi_download would deliver directly after that step, w_j = (m0 / rho_j) W(r), e_j = x_j - x_p, all in fp64,
 *     no self term: n, S, SP, Srho, Sv[3], M1[3], M2[6] (xx, xy, xz, yy, yz, zz), P1[3], R1[3], V1[3][3] as sphmi_sample_point_moments
 *     defines them.  The sums cover EVERY Fluid row within H on the current positions, however long ago the cell list was rebuilt.
 *     n, S, SP, Srho and Sv equal the raw sums behind sphmi_probes_read at the same point and step, bit for bit; the order of summation
 *     depends on the particle order alone, and repeated runs give the same bits.  It differs from that of sphmi_sample_point_moments:
 *     the two agree to rounding (1e-10 of a sum's largest magnitude on fp64 handles), not to the bit.
 *   read: delivers and clears the oldest `capacity` samples recorded since the last read, oldest first: iteration_out / time_out / dt_out
 *     [capacity] as sphmi_probes_read; every other output is [capacity x n_probes x width] with the widths and meanings of
 *     sphmi_sample_point_moments (weight_out 1, count_out 1, sum_pressure_out 1, sum_density_out 1, sum_velocity_out 3, moment1_out 3,
 *     moment2_out 6, moment_pressure_out 3, moment_density_out 3, moment_velocity_out 3 x 3), RAW - nothing is divided by S.  2-D handles
 *     write exact zeros to every slot of the third axis.  Any output pointer may be NULL.  *n_out, *n_dropped, capacity = 0: as
 *     sphmi_group_forces_read.
 *   SPHMI_ERR_STATE: before the upload; read while disabled; rank-mode handles (a process holds one slab of the rows); handles with H < h.
 *   SPHMI_ERR_ARGUMENT: null table, n_probes out of range, a non-finite coordinate, capacity_steps < 1, null n_out.
 * A record is 3 + 31 n_probes doubles: 254 KB at 1024 probes, and the log of a batch of 32 steps 8 MB on the device and as much in
 * page-locked host memory.  Multi-device handles of one process: every sum is linear in the rows, so every slab sums the rows it owns
 * for every probe (ghost copies do not count) and the handle adds the slabs' records in slab order.
 */
int sphmi_probe_moments_enable(sphmi_handle* h, int32_t n_probes, const double* positions /* n_probes x dims */, int64_t capacity_steps);
int sphmi_probe_moments_read(sphmi_handle* h, int64_t capacity, int64_t* iteration_out, double* time_out, double* dt_out,
                             double* weight_out, int64_t* count_out,
                             double* sum_pressure_out, double* sum_density_out, double* sum_velocity_out,
                             double* moment1_out, double* moment2_out,
                             double* moment_pressure_out, double* moment_density_out, double* moment_velocity_out,
                             int64_t* n_out, int64_t* n_dropped);

#ifdef __cplusplus
}
#endif
#endif /* SPHMI_H */
