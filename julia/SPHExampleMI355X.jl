# SPHExampleMI355X.jl — runs SPHExample's hot loop on MI355X GPUs through libsphmi.so (C ABI: include/sphmi.h).
#
#     using SPHExample
#     include("path/to/julia/SPHExampleMI355X.jl")         # before the RunSimulation(...) call; nothing else changes
#
# It adds ONE method: SPHExample.SPHCellList.SimulationLoop for the built-in model tags.  That function is what
# RunSimulation calls once per output interval (src/SPHCellList.jl:883; generic definition :727-733), so example/*.jl,
# RunSimulation itself, logging, ProgressMeter, TimerOutputs, save_particles / save_grid and the VTKHDF writer stay the
# reference's own code.  The method is MORE SPECIFIC than the reference's (concrete Union of tag types in the first
# two arguments): dispatch picks it for ZeroViscosity / ArtificialViscosity / Laminar / LaminarSPS with
# Zero / ZeroGravityLinear / Linear / Complex density diffusion and leaves user-defined SPHViscosity / SPHDensityDiffusion
# subtypes (example/Dambreak2dMDBC.jl:46-66) on the CPU path — no method is overwritten.
#
# What one call costs on the host: the device → host copies of the fields the engine carries (sphmi_download_begin … _end,
# straight into the columns of the StructArray, which are page-locked once) and of the passive columns — the reference's sort!
# permutes all 17 columns, src/SPHCellList.jl:142; the engine carries ten and keeps the others (Type, GravityFactor,
# MotionLimiter, BoundaryBool, GhostNormals, ChunkID, Kernel / KernelGradient without StoreKernelOutput) on the device as opaque
# attached columns (sphmi_attach_columns once, sphmi_download_columns_begin per output): no sortperm, no gather, no per-particle
# loop on the host.  Cells are written in place (a CartesianIndex{D} is D Int64s).  SPHMI_COLUMNS=0 keeps the earlier path: the
# sort as a permutation (sphmi_download_permutation) and ONE host gather per passive column while the copies are in flight.
#
# Environment: SPHMI_LIB (path of libsphmi.so), SPHMI_DEVICE_FLOAT_BYTES (0, default = the library chooses — fp32 kernels when every
# term of the path is continuous: the kernel vanishes at its cut-off, SimKernel.k >= 2, and BMode is NoMDBC (Dambreak3d.jl); fp64
# kernels for DucklingMDBC.jl / MovingSquare2d.jl (k < 2) and every SimpleMDBC run (sphmi_auto_device_float_bytes, include/sphmi.h);
# 4 = fp32; 8 = fp64),
# SPHMI_DEVICES ("0" default; "0,1,2,3,4,5,6,7" = one slab per GPU, halos over RCCL — same calls, see sphmi.h),
# SPHMI_GROUP_FORCES (unset by default; "1,3" = record the force on the Geometries with these GroupMarkers at every step on the
# device — sphmi_group_forces_enable — and collect the series of a run in SPHExampleMI355X.GROUP_FORCES[SimParticles]).
# SPHMI_PROBES (unset by default; "x,y,z;x,y,z" = sample pressure, density and velocity at these fixed points at every step on the
# device — sphmi_probes_enable, `dims` coordinates per point — and collect the series in SPHExampleMI355X.PROBES[SimParticles]).
# SPHMI_PROBE_MOMENTS (unset by default; "x,y,z;x,y,z", the syntax of SPHMI_PROBES = record the raw kernel sums and their first and second
# moments at these fixed points at every step on the device — sphmi_probe_moments_enable, what a linear fit AT a sensor on a wall needs —
# and collect the series in SPHExampleMI355X.PROBE_MOMENTS[SimParticles]).
# SPHMI_BUDGETS (unset by default; "1" = record the energy, momentum and extent budgets of the fluid at every step on the device —
# sphmi_budgets_enable — and collect the series in SPHExampleMI355X.BUDGETS[SimParticles]).
# SPHMI_FLOW_BOXES (unset by default; "lo,lo,lo:hi,hi,hi;…" = record the flow through these half-open control boxes, `dims` bounds on
# either side of the colon, "-Inf" / "Inf" allowed, at every step on the device — sphmi_flow_enable — and collect the series in
# SPHExampleMI355X.FLOW[SimParticles]).
# SPHMI_ENVELOPES (unset by default; "1" = the fluid, or a list of "Fluid", "Fixed", "Moving" = accumulate per particle, at every step on the
# device, the pressure and speed envelopes of the rows of those types — sphmi_envelopes_enable — and keep the newest read, in the row
# order of that output, in SPHExampleMI355X.ENVELOPES[SimParticles]).
# SPHMI_MAPS (unset by default; "origin:spacing:counts[:up_axis]", `dims` numbers per part, "Inf" allowed as a spacing next to a count of 1,
# up_axis zero-based = accumulate per bin of that lattice, at every step on the device, crest, arrival time, wet duration, fill, flux and
# the largest bin-mean speed — sphmi_maps_enable — and keep the newest read in SPHExampleMI355X.MAPS[SimParticles]).
# SPHMI_TRACERS (unset by default; "rows:points[:min_weight]" = follow the particles in these zero-based rows of SimParticles, "0,17,512",
# and advect massless drifters released at these points, "x,y,z;x,y,z", with the flow at every step on the device — either part may be
# empty, min_weight defaults to 0.5 — sphmi_tracers_enable — and collect the series in SPHExampleMI355X.TRACERS[SimParticles]).
#
# EXPERIMENTAL: the build image has no Julia, so this file has never been executed.  struct layout and ABI version
# are asserted against the library at first use (sphmi_create refuses a mismatching struct_size / abi_version).
module SPHExampleMI355X

using SPHExample, StaticArrays, TimerOutputs
import SPHExample.SPHCellList: SimulationLoop, next_output_time

const LIB = get(ENV, "SPHMI_LIB", "libsphmi.so")
const ABI_VERSION = Int32(5)

struct SphmiConfig                       # struct sphmi_config, field for field (include/sphmi.h)
    struct_size::Int32; abi_version::Int32; dims::Int32; host_float_bytes::Int32; device_float_bytes::Int32
    kernel::Int32; viscosity::Int32; density_diffusion::Int32; mdbc::Int32; device::Int32
    shifting::Int32; kernel_output::Int32
    n_particles::Int64; max_cells::Int64
    rho0::Float64; dx::Float64; m0::Float64; alpha::Float64; g::Float64; c0::Float64; gamma::Float64
    delta_phi::Float64; CFL::Float64; Cb::Float64; nu0::Float64
    k::Float64; h::Float64; h_inv::Float64; H::Float64; H_inv::Float64; H2::Float64; alphaD::Float64; eta2::Float64
    blin_constant::Float64; smagorinsky_constant::Float64; cubic_eps::Float64
    n_devices::Int32; slab_axis::Int32; devices::NTuple{16,Int32}
end
mutable struct SphmiProgress
    iteration::Int64; steps_done::Int64; n_rebuilds::Int64; index_counter::Int64
    total_time::Float64; last_dt::Float64; delta_x::Float64
    SphmiProgress() = new(0, 0, 0, 0, 0.0, 0.0, 0.0)
end

const BuiltinViscosity = Union{ZeroViscosity,ArtificialViscosity,Laminar,LaminarSPS}
const BuiltinDDT = Union{ZeroDensityDiffusion,ZeroGravityLinearDensityDiffusion,LinearDensityDiffusion,ComplexDensityDiffusion}
tag(::ZeroViscosity) = Int32(0); tag(::ArtificialViscosity) = Int32(1); tag(::Laminar) = Int32(2); tag(::LaminarSPS) = Int32(3)
tag(::ZeroDensityDiffusion) = Int32(0); tag(::ZeroGravityLinearDensityDiffusion) = Int32(1); tag(::LinearDensityDiffusion) = Int32(2); tag(::ComplexDensityDiffusion) = Int32(3)

# per simulation: the engine handle and the host scratch that lives as long as it (page-locked once, reused every interval)
mutable struct Session
    h::Ptr{Cvoid}
    prev_row::Vector{Int64}              # sphmi_download_permutation: row i now was row prev_row[i] (0-based) at the previous call
    secs::Vector{Float64}                # sphmi_timers at the previous call (device seconds per phase), calls likewise
    calls::Vector{Int64}
    perm::Vector{Int}                    # the same, 1-based
    ucells::Vector{Int64}
    columns::Vector{Any}                 # the passive columns attached to the engine (empty under SPHMI_COLUMNS=0)
    colptrs::Vector{Ptr{Cvoid}}          # their addresses: the table sphmi_download_columns_begin receives
end
const SESSIONS = IdDict{Any,Session}()            # SimParticles (identity) → session
# SPHMI_GROUP_FORCES: the step-resolution series of a run, appended to after every output interval and kept after the run ends —
# iteration, time (at the end of the step), dt, and force[:, g, s] = m₀·Σ Acceleration over the rows of marker g at sample s
mutable struct GroupForceSeries
    markers::Vector{UInt64}
    iteration::Vector{Int64}; time::Vector{Float64}; dt::Vector{Float64}
    force::Array{Float64,3}              # 3 × groups × samples
    dropped::Int64
end
const GROUP_FORCES = IdDict{Any,GroupForceSeries}()
group_force_markers() = UInt64[parse(UInt64, strip(m)) for m in split(get(ENV, "SPHMI_GROUP_FORCES", ""), ",") if !isempty(strip(m))]

# the samples recorded since the last call (sphmi_group_forces_read: first how many wait, then the samples themselves)
function read_group_forces!(h, gf::GroupForceSeries)
    n = Ref{Int64}(0); dropped = Ref{Int64}(0)
    check(h, ccall((:sphmi_group_forces_read, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}, Ref{Int64}),
                   h, 0, C_NULL, C_NULL, C_NULL, C_NULL, n, dropped))
    k = Int(n[]); k == 0 && return nothing
    it = Vector{Int64}(undef, k); t = Vector{Float64}(undef, k); dt = Vector{Float64}(undef, k); f = Array{Float64,3}(undef, 3, length(gf.markers), k)
    GC.@preserve it t dt f check(h, ccall((:sphmi_group_forces_read, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}, Ref{Int64}),
                                          h, k, pointer(it), pointer(t), pointer(dt), pointer(f), n, dropped))
    append!(gf.iteration, it); append!(gf.time, t); append!(gf.dt, dt); gf.force = cat(gf.force, f; dims = 3); gf.dropped += dropped[]
    return nothing
end
# SPHMI_PROBES: the step-resolution series of a run at the probe points, bound like GROUP_FORCES — weight[p, s] = Σ wⱼ (the Shepard sum:
# ≈1 in the fluid, ≈½ at a free surface, 0 in empty space), count[p, s] the rows within H, pressure / density[p, s] and velocity[:, p, s]
# the w-weighted means at probe p and sample s (0 where count is 0)
mutable struct ProbeSeries
    positions::Matrix{Float64}           # dims × probes
    iteration::Vector{Int64}; time::Vector{Float64}; dt::Vector{Float64}
    weight::Matrix{Float64}; count::Matrix{Int64}; pressure::Matrix{Float64}; density::Matrix{Float64}      # probes × samples
    velocity::Array{Float64,3}           # 3 × probes × samples
    dropped::Int64
end
const PROBES = IdDict{Any,ProbeSeries}()
function probe_positions(D, var = "SPHMI_PROBES")
    pts = [parse.(Float64, strip.(split(p, ","))) for p in split(get(ENV, var, ""), ";") if !isempty(strip(p))]
    all(p -> length(p) == D, pts) || error("$var: every point needs $D coordinates (\"x,y;x,y\" / \"x,y,z;x,y,z\")")
    return isempty(pts) ? zeros(Float64, D, 0) : reduce(hcat, pts)
end
function read_probes!(h, pr::ProbeSeries)
    n = Ref{Int64}(0); dropped = Ref{Int64}(0)
    check(h, ccall((:sphmi_probes_read, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}, Ref{Int64}), h, 0, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, n, dropped))
    k = Int(n[]); k == 0 && return nothing
    m = size(pr.positions, 2)
    it = Vector{Int64}(undef, k); t = Vector{Float64}(undef, k); dt = Vector{Float64}(undef, k)
    w = Matrix{Float64}(undef, m, k); c = Matrix{Int64}(undef, m, k); pp = Matrix{Float64}(undef, m, k); rho = Matrix{Float64}(undef, m, k)
    v = Array{Float64,3}(undef, 3, m, k)
    GC.@preserve it t dt w c pp rho v check(h, ccall((:sphmi_probes_read, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}, Ref{Int64}),
                                                     h, k, pointer(it), pointer(t), pointer(dt), pointer(w), pointer(c), pointer(pp), pointer(rho), pointer(v), n, dropped))
    append!(pr.iteration, it); append!(pr.time, t); append!(pr.dt, dt)
    pr.weight = hcat(pr.weight, w); pr.count = hcat(pr.count, c); pr.pressure = hcat(pr.pressure, pp); pr.density = hcat(pr.density, rho)
    pr.velocity = cat(pr.velocity, v; dims = 3); pr.dropped += dropped[]
    return nothing
end
# SPHMI_PROBE_MOMENTS: the step-resolution RAW moment sums at a point set of their own, bound like PROBES — weight[p, s] = Σ w, count[p, s],
# sum_pressure / sum_density[p, s], sum_velocity[:, p, s], and with e = xⱼ − x_p: moment1[:, p, s] = Σ w e, moment2[:, p, s] = Σ w e ⊗ e as
# (xx, xy, xz, yy, yz, zz), moment_pressure / moment_density[:, p, s] = Σ w P e / Σ w ρ e, moment_velocity[b, a, p, s] = Σ w v[a] e[b] (the C
# array's [a][b], column-major).  Nothing is divided by S: the caller solves [[S, M1ᵀ], [M1, M2]] · [a; b] = [Σ w f; Σ w f e] per probe and sample.
mutable struct ProbeMomentSeries
    positions::Matrix{Float64}           # dims × probes
    iteration::Vector{Int64}; time::Vector{Float64}; dt::Vector{Float64}
    weight::Matrix{Float64}; count::Matrix{Int64}; sum_pressure::Matrix{Float64}; sum_density::Matrix{Float64}      # probes × samples
    sum_velocity::Array{Float64,3}; moment1::Array{Float64,3}      # 3 × probes × samples
    moment2::Array{Float64,3}            # 6 × probes × samples
    moment_pressure::Array{Float64,3}; moment_density::Array{Float64,3}      # 3 × probes × samples
    moment_velocity::Array{Float64,4}    # 3 × 3 × probes × samples
    dropped::Int64
end
const PROBE_MOMENTS = IdDict{Any,ProbeMomentSeries}()
function read_probe_moments!(h, pm::ProbeMomentSeries)
    n = Ref{Int64}(0); dropped = Ref{Int64}(0)
    check(h, ccall((:sphmi_probe_moments_read, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}, Ref{Int64}), h, 0, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, n, dropped))
    k = Int(n[]); k == 0 && return nothing
    m = size(pm.positions, 2)
    it = Vector{Int64}(undef, k); t = Vector{Float64}(undef, k); dt = Vector{Float64}(undef, k)
    w = Matrix{Float64}(undef, m, k); c = Matrix{Int64}(undef, m, k); sp = Matrix{Float64}(undef, m, k); sr = Matrix{Float64}(undef, m, k)
    sv = Array{Float64,3}(undef, 3, m, k); m1 = Array{Float64,3}(undef, 3, m, k); m2 = Array{Float64,3}(undef, 6, m, k)
    p1 = Array{Float64,3}(undef, 3, m, k); r1 = Array{Float64,3}(undef, 3, m, k); v1 = Array{Float64,4}(undef, 3, 3, m, k)
    GC.@preserve it t dt w c sp sr sv m1 m2 p1 r1 v1 check(h, ccall((:sphmi_probe_moments_read, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}, Ref{Int64}),
                                                                    h, k, pointer(it), pointer(t), pointer(dt), pointer(w), pointer(c), pointer(sp), pointer(sr), pointer(sv), pointer(m1), pointer(m2), pointer(p1), pointer(r1), pointer(v1), n, dropped))
    append!(pm.iteration, it); append!(pm.time, t); append!(pm.dt, dt)
    pm.weight = hcat(pm.weight, w); pm.count = hcat(pm.count, c); pm.sum_pressure = hcat(pm.sum_pressure, sp); pm.sum_density = hcat(pm.sum_density, sr)
    pm.sum_velocity = cat(pm.sum_velocity, sv; dims = 3); pm.moment1 = cat(pm.moment1, m1; dims = 3); pm.moment2 = cat(pm.moment2, m2; dims = 3)
    pm.moment_pressure = cat(pm.moment_pressure, p1; dims = 3); pm.moment_density = cat(pm.moment_density, r1; dims = 3)
    pm.moment_velocity = cat(pm.moment_velocity, v1; dims = 4); pm.dropped += dropped[]
    return nothing
end
# SPHMI_BUDGETS: the step-resolution budgets of the fluid, bound like GROUP_FORCES — count[s] Fluid rows, energy[:, s] (kinetic, potential,
# compressive), momentum[:, s], angular[:, s] (about the origin), centre[:, s] (of mass), extremes[:, s] (largest speed, smallest and largest
# density) and box[:, s] (min x[1:3], max x[1:3]; box[4, :] is the wave front of a dam break that runs towards +x) at sample s
mutable struct BudgetSeries
    iteration::Vector{Int64}; time::Vector{Float64}; dt::Vector{Float64}
    count::Vector{Int64}
    energy::Matrix{Float64}; momentum::Matrix{Float64}; angular::Matrix{Float64}; centre::Matrix{Float64}; extremes::Matrix{Float64}      # 3 × samples
    box::Matrix{Float64}                 # 6 × samples
    dropped::Int64
end
const BUDGETS = IdDict{Any,BudgetSeries}()
budgets_wanted() = !(strip(get(ENV, "SPHMI_BUDGETS", "")) in ("", "0"))
function read_budgets!(h, bs::BudgetSeries)
    n = Ref{Int64}(0); dropped = Ref{Int64}(0)
    check(h, ccall((:sphmi_budgets_read, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}, Ref{Int64}),
                   h, 0, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, n, dropped))
    k = Int(n[]); k == 0 && return nothing
    it = Vector{Int64}(undef, k); t = Vector{Float64}(undef, k); dt = Vector{Float64}(undef, k); c = Vector{Int64}(undef, k)
    en = Matrix{Float64}(undef, 3, k); mom = Matrix{Float64}(undef, 3, k); ang = Matrix{Float64}(undef, 3, k); cen = Matrix{Float64}(undef, 3, k)
    ext = Matrix{Float64}(undef, 3, k); bx = Matrix{Float64}(undef, 6, k)
    GC.@preserve it t dt c en mom ang cen ext bx check(h, ccall((:sphmi_budgets_read, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}, Ref{Int64}),
                                                            h, k, pointer(it), pointer(t), pointer(dt), pointer(c), pointer(en), pointer(mom), pointer(ang), pointer(cen), pointer(ext), pointer(bx), n, dropped))
    append!(bs.iteration, it); append!(bs.time, t); append!(bs.dt, dt); append!(bs.count, c)
    bs.energy = hcat(bs.energy, en); bs.momentum = hcat(bs.momentum, mom); bs.angular = hcat(bs.angular, ang); bs.centre = hcat(bs.centre, cen)
    bs.extremes = hcat(bs.extremes, ext); bs.box = hcat(bs.box, bx); bs.dropped += dropped[]
    return nothing
end
# SPHMI_FLOW_BOXES: the step-resolution flow through control boxes, bound like BUDGETS — count[b, s] Fluid rows inside box b after sample s,
# volume[b, s], momentum[:, b, s], entered[b, s] and left[b, s] (rows that crossed into / out of the box during the step)
mutable struct FlowSeries
    lo::Matrix{Float64}; hi::Matrix{Float64}            # dims × boxes
    iteration::Vector{Int64}; time::Vector{Float64}; dt::Vector{Float64}
    count::Matrix{Int64}; volume::Matrix{Float64}; momentum::Array{Float64,3}; entered::Matrix{Int64}; left::Matrix{Int64}
    dropped::Int64
end
const FLOW = IdDict{Any,FlowSeries}()
function flow_boxes(D)
    sides = [[parse.(Float64, strip.(split(side, ","))) for side in split(b, ":")] for b in split(get(ENV, "SPHMI_FLOW_BOXES", ""), ";") if !isempty(strip(b))]
    all(b -> length(b) == 2 && length(b[1]) == D && length(b[2]) == D, sides) || error("SPHMI_FLOW_BOXES: every box is \"lo:hi\" with $D bounds on either side")
    isempty(sides) && return zeros(Float64, D, 0), zeros(Float64, D, 0)
    return reduce(hcat, [b[1] for b in sides]), reduce(hcat, [b[2] for b in sides])
end
function read_flow!(h, fs::FlowSeries)
    n = Ref{Int64}(0); dropped = Ref{Int64}(0)
    check(h, ccall((:sphmi_flow_read, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ref{Int64}, Ref{Int64}),
                   h, 0, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, n, dropped))
    k = Int(n[]); k == 0 && return nothing
    m = size(fs.lo, 2)
    it = Vector{Int64}(undef, k); t = Vector{Float64}(undef, k); dt = Vector{Float64}(undef, k)
    c = Matrix{Int64}(undef, m, k); vol = Matrix{Float64}(undef, m, k); mom = Array{Float64,3}(undef, 3, m, k); en = Matrix{Int64}(undef, m, k); le = Matrix{Int64}(undef, m, k)
    GC.@preserve it t dt c vol mom en le check(h, ccall((:sphmi_flow_read, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}, Ref{Int64}, Ref{Int64}),
                                                       h, k, pointer(it), pointer(t), pointer(dt), pointer(c), pointer(vol), pointer(mom), pointer(en), pointer(le), n, dropped))
    append!(fs.iteration, it); append!(fs.time, t); append!(fs.dt, dt)
    fs.count = hcat(fs.count, c); fs.volume = hcat(fs.volume, vol); fs.momentum = cat(fs.momentum, mom; dims = 3)
    fs.entered = hcat(fs.entered, en); fs.left = hcat(fs.left, le); fs.dropped += dropped[]
    return nothing
end
# SPHMI_ENVELOPES: what every particle has experienced since the session opened, bound like FLOW — but a state, not a series: every output
# REPLACES the arrays (row i is particle i of that output): p_max, t_p_max, p_min, impulse (Σ P·dt), square (Σ P²·dt), loaded (Σ dt over
# steps with P > 0), speed_max and t_arrival (Inf: never loaded); steps, t_begin, t_end, duration describe the window
mutable struct Envelopes
    mask::Int32
    steps::Int64; t_begin::Float64; t_end::Float64; duration::Float64
    p_max::Vector{Float64}; t_p_max::Vector{Float64}; p_min::Vector{Float64}; impulse::Vector{Float64}; square::Vector{Float64}
    loaded::Vector{Float64}; speed_max::Vector{Float64}; t_arrival::Vector{Float64}
end
const ENVELOPES = IdDict{Any,Envelopes}()
const ENVELOPE_TYPES = Dict("fluid" => 1, "fixed" => 2, "moving" => 3)
function envelopes_mask()
    asked = lowercase.(strip.(split(get(ENV, "SPHMI_ENVELOPES", ""), ",")))
    asked = [a for a in asked if !(a in ("", "0"))]
    isempty(asked) && return Int32(0)
    all(a -> a == "1" || haskey(ENVELOPE_TYPES, a), asked) || error("SPHMI_ENVELOPES: \"1\" (the fluid) or a list of Fluid, Fixed, Moving")
    return Int32(reduce(|, [1 << (a == "1" ? 1 : ENVELOPE_TYPES[a]) for a in asked]))
end
function envelopes_enable(h, mask::Integer)
    check(h, ccall((:sphmi_envelopes_enable, LIB), Cint, (Ptr{Cvoid}, Int32), h, Int32(mask)))
    return nothing
end
function envelopes_read(h, n::Integer)
    steps = Ref{Int64}(0); window = zeros(3)
    a = [Vector{Float64}(undef, n) for _ in 1:8]
    GC.@preserve window a check(h, ccall((:sphmi_envelopes_read, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                         h, steps, pointer(window), pointer(a[1]), pointer(a[2]), pointer(a[3]), pointer(a[4]), pointer(a[5]), pointer(a[6]), pointer(a[7]), pointer(a[8])))
    return steps[], window, a
end
function read_envelopes!(h, en::Envelopes, n::Integer)
    en.steps, w, a = envelopes_read(h, n)
    en.t_begin, en.t_end, en.duration = w
    en.p_max, en.t_p_max, en.p_min, en.impulse, en.square, en.loaded, en.speed_max, en.t_arrival = a
    return nothing
end
# SPHMI_TRACERS: where the water goes, bound like PROBES — particles[:, s, k] = (x, y, z, vx, vy, vz, ρ, P) of tracked particle s after sample k,
# drifters[:, p, k] = (X, Y, Z, S, SP, Sρ, Svx, Svy, Svz, n) of drifter p: the position the raw sums of sample k were taken at, BEFORE its move;
# position[:, p] is where the drifters are now (a drifter moves by (Sv / S)·dt where S ≥ min_weight and stays where it is dry)
mutable struct TracerSeries
    rows::Vector{Int64}                  # zero-based rows at the enable
    released::Matrix{Float64}            # dims × drifters
    min_weight::Float64
    iteration::Vector{Int64}; time::Vector{Float64}; dt::Vector{Float64}
    particles::Array{Float64,3}          # 8 × tracked × samples
    drifters::Array{Float64,3}           # 10 × drifters × samples
    position::Matrix{Float64}            # 3 × drifters
    dropped::Int64
end
const TRACERS = IdDict{Any,TracerSeries}()
function tracer_spec(D)
    spec = strip(get(ENV, "SPHMI_TRACERS", ""))
    (isempty(spec) || spec == "0") && return nothing
    parts = split(spec, ":")
    2 <= length(parts) <= 3 || error("SPHMI_TRACERS: \"rows:points[:min_weight]\", either of the first two may be empty")
    rows = Int64[parse(Int64, strip(r)) for r in split(parts[1], ",") if !isempty(strip(r))]
    pts = [parse.(Float64, strip.(split(q, ","))) for q in split(parts[2], ";") if !isempty(strip(q))]
    all(q -> length(q) == D, pts) || error("SPHMI_TRACERS: every point needs $D coordinates")
    (isempty(rows) && isempty(pts)) && return nothing
    weight = length(parts) == 3 ? parse(Float64, strip(parts[3])) : 0.5
    return rows, (isempty(pts) ? zeros(Float64, D, 0) : reduce(hcat, pts)), weight
end
function tracers_enable(h, rows::Vector{Int64}, points::Matrix{Float64}, min_weight::Float64)
    GC.@preserve rows points check(h, ccall((:sphmi_tracers_enable, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Int64}, Int32, Ptr{Float64}, Float64, Int64),
                                            h, Int32(length(rows)), isempty(rows) ? Ptr{Int64}(C_NULL) : pointer(rows), Int32(size(points, 2)),
                                            isempty(points) ? Ptr{Float64}(C_NULL) : pointer(points), min_weight, 1 << 16))
    return nothing
end
function read_tracers!(h, tr::TracerSeries)
    np = length(tr.rows); nd = size(tr.released, 2); chunk = 256
    n = Ref{Int64}(0); dropped = Ref{Int64}(0)
    it = Vector{Int64}(undef, chunk); t = Vector{Float64}(undef, chunk); dt = Vector{Float64}(undef, chunk)
    pv = Array{Float64,3}(undef, 8, np, chunk); dv = Array{Float64,3}(undef, 10, nd, chunk); x = zeros(Float64, 3, nd)
    while true                           # the oldest `chunk` samples per call until none is left: one call site, no question first
        GC.@preserve it t dt pv dv x check(h, ccall((:sphmi_tracers_read, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ref{Int64}, Ref{Int64}),
                                                   h, chunk, pointer(it), pointer(t), pointer(dt), pointer(pv), pointer(dv), pointer(x), n, dropped))
        k = Int(n[])
        append!(tr.iteration, it[1:k]); append!(tr.time, t[1:k]); append!(tr.dt, dt[1:k])
        tr.particles = cat(tr.particles, pv[:, :, 1:k]; dims = 3); tr.drifters = cat(tr.drifters, dv[:, :, 1:k]; dims = 3)
        tr.dropped += dropped[]
        k < chunk && break
    end
    tr.position = x
    return nothing
end
# SPHMI_MAPS: what every bin of a lattice has experienced since the session opened, bound like ENVELOPES — a state, not a series: every
# output REPLACES the arrays.  Arrays are indexed [k0, k1[, k2]] (x fastest: Julia's column-major order IS the bin order), flux and
# last_velocity_sum as 3 × counts…; speed2_max is the SQUARE of the largest bin-mean speed; t_arrival is Inf in a bin that never got wet
mutable struct Maps
    origin::Vector{Float64}; spacing::Vector{Float64}; counts::Vector{Int64}; up_axis::Int32
    steps::Int64; t_begin::Float64; t_end::Float64; duration::Float64
    top_max::Array{Float64}; t_top_max::Array{Float64}; bottom_min::Array{Float64}; t_arrival::Array{Float64}; wet::Array{Float64}; fill::Array{Float64}
    flux::Array{Float64}; speed2_max::Array{Float64}; t_speed2_max::Array{Float64}; n_max::Array{Float64}
    last_n::Array{Int64}; last_top::Array{Float64}; last_bottom::Array{Float64}; last_velocity_sum::Array{Float64}
end
const MAPS = IdDict{Any,Maps}()
function maps_lattice(D)
    parts = [strip.(split(part, ",")) for part in split(get(ENV, "SPHMI_MAPS", ""), ":") if !isempty(strip(part))]
    isempty(parts) && return nothing
    (length(parts) in (3, 4) && all(k -> length(parts[k]) == D, 1:3) && (length(parts) == 3 || length(parts[4]) == 1)) ||
        error("SPHMI_MAPS: \"origin:spacing:counts[:up_axis]\" with $D numbers in each of the first three parts")
    up = length(parts) == 4 ? parse(Int32, parts[4][1]) : Int32(D - 1)
    return parse.(Float64, parts[1]), parse.(Float64, parts[2]), parse.(Int64, parts[3]), up
end
function maps_enable(h, origin::Vector{Float64}, spacing::Vector{Float64}, counts::Vector{Int64}, up_axis::Integer)
    GC.@preserve origin spacing counts check(h, ccall((:sphmi_maps_enable, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Int32),
                                                       h, pointer(origin), pointer(spacing), pointer(counts), Int32(up_axis)))
    return nothing
end
function maps_disable(h)
    check(h, ccall((:sphmi_maps_disable, LIB), Cint, (Ptr{Cvoid},), h))
    return nothing
end
function maps_read(h, counts::Vector{Int64})
    dims = Tuple(Int.(counts))
    steps = Ref{Int64}(0); window = zeros(3)
    a = [Array{Float64}(undef, k == 7 ? (3, dims...) : dims) for k in 1:10]
    ln = Array{Int64}(undef, dims); lt = Array{Float64}(undef, dims); lb = Array{Float64}(undef, dims); ls = Array{Float64}(undef, (3, dims...))
    GC.@preserve window a ln lt lb ls check(h, ccall((:sphmi_maps_read, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                                     h, steps, pointer(window), pointer(a[1]), pointer(a[2]), pointer(a[3]), pointer(a[4]), pointer(a[5]), pointer(a[6]), pointer(a[7]), pointer(a[8]), pointer(a[9]), pointer(a[10]), pointer(ln), pointer(lt), pointer(lb), pointer(ls)))
    return steps[], window, a, (ln, lt, lb, ls)
end
function read_maps!(h, mp::Maps)
    mp.steps, w, a, last = maps_read(h, mp.counts)
    mp.t_begin, mp.t_end, mp.duration = w
    mp.top_max, mp.t_top_max, mp.bottom_min, mp.t_arrival, mp.wet, mp.fill, mp.flux, mp.speed2_max, mp.t_speed2_max, mp.n_max = a
    mp.last_n, mp.last_top, mp.last_bottom, mp.last_velocity_sum = last
    return nothing
end
# The probes' sums at every node of a regular lattice, evaluated on the state the session holds NOW (sphmi_sample_grid): node (i, j[, k])
# lies at origin .+ (i, j[, k]) .* spacing, zero-based.  Returns arrays indexed [i, j[, k]] (x fastest: Julia's column-major order IS the
# node order), velocity as 3 × nx × ny[ × nz].  Call it from an output callback, i.e. between two SimulationLoop calls, after the first step.
function sample_grid(P, origin::Vector{Float64}, spacing::Vector{Float64}, counts::Vector{Int64})
    h = SESSIONS[P].h
    dims = Tuple(Int.(counts))
    w = Array{Float64}(undef, dims); c = Array{Int64}(undef, dims); pp = Array{Float64}(undef, dims); rho = Array{Float64}(undef, dims)
    v = Array{Float64}(undef, (3, dims...))
    GC.@preserve origin spacing counts w c pp rho v check(h, ccall((:sphmi_sample_grid, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                                                       h, pointer(origin), pointer(spacing), pointer(counts), pointer(w), pointer(c), pointer(pp), pointer(rho), pointer(v)))
    return (weight = w, count = c, pressure = pp, density = rho, velocity = v)
end
# The same sums at ARBITRARY points, evaluated on the state the session holds NOW (sphmi_sample_points): positions is dims × n, column p
# the coordinates of point p (column-major: the rows the library reads) — panel centroids, mesh nodes, a ring of sensors.  Returns vectors
# of length n in the caller's order, velocity as 3 × n; a point's result does not depend on the other points of the call.  Call it from an
# output callback, i.e. between two SimulationLoop calls, after the first step.
function sample_points(P, positions::Matrix{Float64})
    h = SESSIONS[P].h
    n = size(positions, 2)
    w = Vector{Float64}(undef, n); c = Vector{Int64}(undef, n); pp = Vector{Float64}(undef, n); rho = Vector{Float64}(undef, n)
    v = Matrix{Float64}(undef, 3, n)
    GC.@preserve positions w c pp rho v check(h, ccall((:sphmi_sample_points, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                                      h, Int64(n), pointer(positions), pointer(w), pointer(c), pointer(pp), pointer(rho), pointer(v)))
    return (weight = w, count = c, pressure = pp, density = rho, velocity = v)
end
# The RAW kernel and gradient sums at arbitrary points, evaluated on the state the session holds NOW (sphmi_sample_point_gradients):
# positions is dims × n as for sample_points.  weight S, count n, sum_pressure, sum_density (length n), sum_velocity, grad_weight,
# grad_pressure, grad_density (3 × n) and grad_velocity (3 × 3 × n, entry [b, a, p] = Σ V_j v_j[a] ∂W/∂x_b: column-major, the derivative
# axis first).  Nothing is divided by S: ∇A ≈ (GA − (SA / S) · G) / S is the caller's.  Multi-device sessions of one process deliver the
# sums over all slabs.  Call it from an output callback, after the first step.
function sample_point_gradients(P, positions::Matrix{Float64})
    h = SESSIONS[P].h
    n = size(positions, 2)
    w = Vector{Float64}(undef, n); c = Vector{Int64}(undef, n); sp = Vector{Float64}(undef, n); sr = Vector{Float64}(undef, n)
    sv = Matrix{Float64}(undef, 3, n); g = Matrix{Float64}(undef, 3, n); gp = Matrix{Float64}(undef, 3, n); gr = Matrix{Float64}(undef, 3, n)
    gv = Array{Float64, 3}(undef, 3, 3, n)
    GC.@preserve positions w c sp sr sv g gp gr gv check(h, ccall((:sphmi_sample_point_gradients, LIB), Cint,
                                                             (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                                             h, Int64(n), pointer(positions), pointer(w), pointer(c), pointer(sp), pointer(sr), pointer(sv), pointer(g), pointer(gp), pointer(gr), pointer(gv)))
    return (weight = w, count = c, sum_pressure = sp, sum_density = sr, sum_velocity = sv, grad_weight = g, grad_pressure = gp, grad_density = gr, grad_velocity = gv)
end
# The RAW kernel sums and their first and second moments at arbitrary points, evaluated on the state the session holds NOW
# (sphmi_sample_point_moments): positions is dims × n as for sample_points.  With w_j = (m0 / ρ_j) W(r) and e_j = x_j − x: weight S,
# count n, sum_pressure, sum_density (length n), sum_velocity, moment1 Σ w e, moment_pressure Σ w P e, moment_density Σ w ρ e (3 × n),
# moment2 (6 × n: xx, xy, xz, yy, yz, zz of Σ w e ⊗ e) and moment_velocity (3 × 3 × n, entry [b, a, p] = Σ w v[a] e[b]: column-major, the
# offset axis first).  Nothing is divided by S: the linear fit [[S, M1ᵀ], [M1, M2]] · [a; b] = [Σ w f; Σ w f e] is the caller's.
# Multi-device sessions of one process deliver the sums over all slabs.  Call it from an output callback, after the first step.
function sample_point_moments(P, positions::Matrix{Float64})
    h = SESSIONS[P].h
    n = size(positions, 2)
    w = Vector{Float64}(undef, n); c = Vector{Int64}(undef, n); sp = Vector{Float64}(undef, n); sr = Vector{Float64}(undef, n)
    sv = Matrix{Float64}(undef, 3, n); m1 = Matrix{Float64}(undef, 3, n); m2 = Matrix{Float64}(undef, 6, n); p1 = Matrix{Float64}(undef, 3, n)
    r1 = Matrix{Float64}(undef, 3, n); v1 = Array{Float64, 3}(undef, 3, 3, n)
    GC.@preserve positions w c sp sr sv m1 m2 p1 r1 v1 check(h, ccall((:sphmi_sample_point_moments, LIB), Cint,
                                                             (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                                             h, Int64(n), pointer(positions), pointer(w), pointer(c), pointer(sp), pointer(sr), pointer(sv), pointer(m1), pointer(m2), pointer(p1), pointer(r1), pointer(v1)))
    return (weight = w, count = c, sum_pressure = sp, sum_density = sr, sum_velocity = sv, moment1 = m1, moment2 = m2, moment_pressure = p1, moment_density = r1, moment_velocity = v1)
end
# The first crossing of S = level along rays, found on the state the session holds NOW (sphmi_cast_rays): origins and directions are
# dims × n, t_end a number or a vector of length n; step is the march step in units of |d| (say h / 2); mode is :enter, :leave or :any.  status (bit 0: found, bit 1:
# the ray starts inside), interval (k, or −1), bracket (2 × n), point (3 × n: the inside end), weight, count, sum_pressure, sum_density
# (length n) and sum_velocity (3 × n) — the raw sums of sample_point_gradients at point.  NaN brackets and points where nothing was hit.
# Single-device sessions; call it from an output callback, after the first step.
function cast_rays(P, origins::Matrix{Float64}, directions::Matrix{Float64}, t_end; step, t_begin = 0.0, level = 0.5, mode = :enter)
    h = SESSIONS[P].h
    n = size(origins, 2)
    size(directions) == size(origins) || error("cast_rays: origins and directions are both dims × n")
    tb = t_begin isa Number ? fill(Float64(t_begin), n) : Vector{Float64}(t_begin)
    te = t_end isa Number ? fill(Float64(t_end), n) : Vector{Float64}(t_end)
    (length(tb) == n && length(te) == n) || error("cast_rays: t_begin and t_end are numbers or vectors of length n")
    dt = Float64(step)
    md = Int32(Dict(:enter => 0, :leave => 1, :any => 2)[mode])
    st = Vector{Int32}(undef, n); iv = Vector{Int64}(undef, n); br = Matrix{Float64}(undef, 2, n); pt = Matrix{Float64}(undef, 3, n)
    w = Vector{Float64}(undef, n); c = Vector{Int64}(undef, n); sp = Vector{Float64}(undef, n); sr = Vector{Float64}(undef, n)
    sv = Matrix{Float64}(undef, 3, n)
    GC.@preserve origins directions tb te st iv br pt w c sp sr sv check(h, ccall((:sphmi_cast_rays, LIB), Cint,
                                                             (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Float64, Float64, Int32, Ptr{Int32}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                                             h, Int64(n), pointer(origins), pointer(directions), pointer(tb), pointer(te), dt, Float64(level), md, pointer(st), pointer(iv), pointer(br), pointer(pt), pointer(w), pointer(c), pointer(sp), pointer(sr), pointer(sv)))
    return (status = st, interval = iv, bracket = br, point = pt, weight = w, count = c, sum_pressure = sp, sum_density = sr, sum_velocity = sv)
end
# Differential fields at the particles, evaluated on the state the session holds NOW (sphmi_particle_fields): row i is row i of the next
# download.  count[i] rows within H, shepard[i], div_r[i] (≈ D inside, lower at a free surface), div_v[i], normal[:, i] and vorticity[:, i]
# (3 × n; 2-D: only vorticity[3, :] and normal[1:2, :] are non-zero).  Single-device sessions; call it from an output callback, after the first step.
function particle_fields(P)
    h = SESSIONS[P].h
    n = length(P)
    c = Vector{Int64}(undef, n); s = Vector{Float64}(undef, n); nrm = Matrix{Float64}(undef, 3, n)
    dr = Vector{Float64}(undef, n); dv = Vector{Float64}(undef, n); w = Matrix{Float64}(undef, 3, n)
    GC.@preserve c s nrm dr dv w check(h, ccall((:sphmi_particle_fields, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                                                h, pointer(c), pointer(s), pointer(nrm), pointer(dr), pointer(dv), pointer(w)))
    return (count = c, shepard = s, normal = nrm, div_r = dr, div_v = dv, vorticity = w)
end
# The neighbour list of every row on the state the session holds NOW (sphmi_neighbors_build / _read / _release): row i (1-based) of the
# next download lists neighbors[offsets[i] + 1 : offsets[i + 1]], every other row within H, ascending.  Both arrays are the library's RAW
# 0-BASED values — offsets[1] == 0 and an entry j names row j + 1 of the StructArray.  Single-device sessions; from an output callback.
function neighbor_list(P; half::Bool = false)
    h = SESSIONS[P].h
    rows = Ref{Int64}(0); pairs = Ref{Int64}(0)
    check(h, ccall((:sphmi_neighbors_build, LIB), Cint, (Ptr{Cvoid}, Int32, Ref{Int64}, Ref{Int64}), h, half ? 1 : 0, rows, pairs))
    offsets = Vector{Int64}(undef, rows[] + 1); neighbors = Vector{Int32}(undef, pairs[])
    GC.@preserve offsets neighbors check(h, ccall((:sphmi_neighbors_read, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}), h, pointer(offsets), pointer(neighbors)))
    check(h, ccall((:sphmi_neighbors_release, LIB), Cint, (Ptr{Cvoid},), h))
    return (offsets = offsets, neighbors = neighbors)
end
# The free surface as a mesh on the state the session holds NOW (sphmi_isosurface_build / _read / _release): the surface S == level of
# the Shepard sum on the lattice sample_grid takes.  vertices is 3 × nv, elements D × ne — triangles in 3-D (normals out of the fluid),
# segments in 2-D (the fluid to the left) — with the library's RAW 0-BASED vertex indices; pressure [nv] and velocity 3 × nv are the
# lattice means interpolated to the vertices.  Single-device sessions; from an output callback, after the first step.
function isosurface(P, origin::Vector{Float64}, spacing::Vector{Float64}, counts::Vector{Int64}; level::Float64 = 0.5)
    h = SESSIONS[P].h
    nv = Ref{Int64}(0); ne = Ref{Int64}(0)
    GC.@preserve origin spacing counts check(h, ccall((:sphmi_isosurface_build, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Float64, Ref{Int64}, Ref{Int64}),
                                                       h, pointer(origin), pointer(spacing), pointer(counts), level, nv, ne))
    vertices = Matrix{Float64}(undef, 3, nv[]); elements = Matrix{Int32}(undef, length(counts), ne[])
    pp = Vector{Float64}(undef, nv[]); v = Matrix{Float64}(undef, 3, nv[])
    GC.@preserve vertices elements pp v check(h, ccall((:sphmi_isosurface_read, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Int32}, Ptr{Float64}, Ptr{Float64}),
                                                        h, pointer(vertices), pointer(elements), pointer(pp), pointer(v)))
    check(h, ccall((:sphmi_isosurface_release, LIB), Cint, (Ptr{Cvoid},), h))
    return (vertices = vertices, elements = elements, pressure = pp, velocity = v)
end
# The connected bodies of the fluid on the state the session holds NOW (sphmi_components_build / _read / _release): rows of the Types
# named (Fluid = 1, Fixed = 2, Moving = 3) are linked within `link` (at most SimKernel.H); label[i] is the component of row i of the next
# download or -1, first_row / count / box (6 × C: min x, y, z, max x, y, z) describe the components, numbered in ascending first row.
# label and first_row are the library's RAW 0-BASED values.  Single-device sessions; from an output callback, after the first step.
# (The build goes through @ccall: its mask is the header's only 32-bit unsigned argument, a width the table of
# tests/test_julia_shim.py does not hold; tests/test_components_host.py holds this call to its prototype.)
function components(P, link::Float64; types = (1,))
    h = SESSIONS[P].h
    mask = reduce(|, (UInt32(1) << t for t in types); init = UInt32(0))
    rows = Ref{Int64}(0); comps = Ref{Int64}(0)
    check(h, @ccall LIB.sphmi_components_build(h::Ptr{Cvoid}, link::Float64, mask::UInt32, rows::Ref{Int64}, comps::Ref{Int64})::Cint)
    label = Vector{Int32}(undef, rows[]); first_row = Vector{Int32}(undef, comps[]); count = Vector{Int32}(undef, comps[])
    box = Matrix{Float64}(undef, 6, comps[])
    GC.@preserve label first_row count box check(h, ccall((:sphmi_components_read, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float64}),
                                                            h, pointer(label), pointer(first_row), pointer(count), pointer(box)))
    check(h, ccall((:sphmi_components_release, LIB), Cint, (Ptr{Cvoid},), h))
    return (label = label, first_row = first_row, count = count, box = box)
end
# A selected subset of the rows of the state the session holds NOW, compacted on the device (sphmi_select_build / _read / _download /
# _release): only the selected rows cross the bus.  Every clause that is given must hold: `types` (Fluid = 1, Fixed = 2, Moving = 3),
# `lo` / `hi` (D × n_boxes, half-open lo <= x < hi per axis, ±Inf allowed; the row lies in SOME box), `markers`, ID % stride == phase
# (the same particles through every sort), `field` (0 none, 1 Density, 2 Pressure, 3 the squared speed) within [field_lo, field_hi],
# `mask` (one byte per row of the next download, non-zero keeps).  rows are the library's RAW 0-BASED row numbers, ascending; position
# and velocity are D × n, in the float type of the StructArray.  Single-device sessions; from an output callback, any time after the upload.
struct SphmiSelection
    type_mask::UInt32; n_boxes::Int32
    box_lo::Ptr{Float64}; box_hi::Ptr{Float64}
    n_markers::Int32
    markers::Ptr{UInt64}
    id_stride::Int64; id_phase::Int64
    field::Int32
    field_lo::Float64; field_hi::Float64
    row_mask::Ptr{UInt8}
end
function select_rows(P; types = (1, 2, 3), lo::Matrix{Float64} = zeros(0, 0), hi::Matrix{Float64} = zeros(0, 0), markers::Vector{UInt64} = UInt64[],
                     stride::Integer = 1, phase::Integer = 0, field::Integer = 0, field_lo::Float64 = -Inf, field_hi::Float64 = Inf,
                     mask::Vector{UInt8} = UInt8[])
    h = SESSIONS[P].h
    F = eltype(P.Density)
    size(lo) == size(hi) || error("select_rows: lo and hi are both dims × n_boxes")
    isempty(mask) || length(mask) == length(P) || error("select_rows: the mask holds one byte per row")
    tmask = reduce(|, (UInt32(1) << (t - 1) for t in types); init = UInt32(0))
    nrows = Ref{Int64}(0); kept = Ref{Int64}(0)
    GC.@preserve lo hi markers mask begin
        sel = Ref(SphmiSelection(tmask, size(lo, 2), size(lo, 2) > 0 ? pointer(lo) : C_NULL, size(hi, 2) > 0 ? pointer(hi) : C_NULL,
                                 length(markers), isempty(markers) ? C_NULL : pointer(markers), stride, phase, field, field_lo, field_hi,
                                 isempty(mask) ? C_NULL : pointer(mask)))
        check(h, ccall((:sphmi_select_build, LIB), Cint, (Ptr{Cvoid}, Ref{SphmiSelection}, Ref{Int64}, Ref{Int64}), h, sel, nrows, kept))
    end
    n = kept[]; D = length(first(P.Position))
    rows = Vector{Int32}(undef, n); x = Matrix{F}(undef, D, n); v = Matrix{F}(undef, D, n); rho = Vector{F}(undef, n); pp = Vector{F}(undef, n)
    id = Vector{Int64}(undef, n); ty = Vector{UInt8}(undef, n); grp = Vector{UInt64}(undef, n)
    GC.@preserve rows check(h, ccall((:sphmi_select_read, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}), h, pointer(rows)))
    GC.@preserve x v rho pp id ty grp check(h, ccall((:sphmi_select_download, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}, Ptr{UInt64}, Ptr{Cvoid}, Ptr{Int64}),
        h, pointer(x), pointer(v), C_NULL, pointer(rho), pointer(pp), pointer(id), pointer(ty), pointer(grp), C_NULL, C_NULL))
    check(h, ccall((:sphmi_select_release, LIB), Cint, (Ptr{Cvoid},), h))
    return (rows = rows, position = x, velocity = v, density = rho, pressure = pp, id = id, type = ty, group_marker = grp)
end
atexit(() -> foreach(s -> ccall((:sphmi_destroy, LIB), Cint, (Ptr{Cvoid},), s.h), values(SESSIONS)))

function check(h, rc)
    rc == 0 || error("libsphmi status $rc: " * unsafe_string(ccall((:sphmi_last_error, LIB), Cstring, (Ptr{Cvoid},), h)))
end

# the columns sphmi_download writes every interval: page-locked once (the arrays of the StructArray live for the whole run;
# a multi-device handle accepts the call and stages through its own buffers).  Pinning is an optimisation only — an array that
# cannot be page-locked (locked-memory limit, a range the runtime already knows) is filled through the engine's bounce buffer
# in sphmi_download_end — so a refusal is not an error.
pin(h, a::Array) = isempty(a) || ccall((:sphmi_host_register, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), h, pointer(a), sizeof(a))

function open_session(SimDensityDiffusion, SimViscosity, SimKernel, SimMetaData::SimulationMetaData{D,T,S,K,B,L}, SimConstants, P, MotionDefinition) where {D,T,S,K,B,L}
    devs = parse.(Int32, split(get(ENV, "SPHMI_DEVICES", "0"), ","))
    N = length(P)
    cfg = SphmiConfig(sizeof(SphmiConfig), ABI_VERSION, D, sizeof(T), parse(Int32, get(ENV, "SPHMI_DEVICE_FLOAT_BYTES", "0")),
                      SimKernel.kernel isa CubicSpline ? 1 : 0, tag(SimViscosity), tag(SimDensityDiffusion), B <: SimpleMDBC ? 1 : 0,
                      devs[1], S <: PlanarShifting ? 1 : 0, K <: StoreKernelOutput ? 1 : 0, N, 0,
                      SimConstants.ρ₀, SimConstants.dx, SimConstants.m₀, SimConstants.α, SimConstants.g, SimConstants.c₀,
                      SimConstants.γ, SimConstants.δᵩ, SimConstants.CFL, SimConstants.Cb, SimConstants.ν₀,
                      SimKernel.k, SimKernel.h, SimKernel.h⁻¹, SimKernel.H, SimKernel.H⁻¹, SimKernel.H², SimKernel.αD, SimKernel.η²,
                      SimConstants.BlinConstant, SimConstants.SmagorinskyConstant,
                      SimKernel.kernel isa CubicSpline ? Float64(SimKernel.kernel.eps) : 0.0,
                      length(devs), 0, ntuple(i -> i <= length(devs) ? devs[i] : Int32(0), 16))
    href = Ref{Ptr{Cvoid}}(C_NULL)
    check(C_NULL, ccall((:sphmi_create, LIB), Cint, (Ref{SphmiConfig}, Ref{Ptr{Cvoid}}), cfg, href))
    h = href[]
    try                                   # (from here on the handle exists and is not yet in SESSIONS: an error must not leak it)
    for (group, m) in enumerate(MotionDefinition)                                  # RunSimulation's table, :846-850
        m === nothing && continue
        dir = Float64[m.Direction...]
        GC.@preserve dir check(h, ccall((:sphmi_set_motion, LIB), Cint, (Ptr{Cvoid}, UInt64, Float64, Float64, Float64, Ptr{Float64}),
                                        h, UInt64(group), Float64(m.Velocity), Float64(m.StartTime), Float64(m.Duration), pointer(dir)))
    end
    typ = Vector{UInt8}(UInt8.(P.Type))
    GC.@preserve P typ check(h, ccall((:sphmi_upload, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Int64}, Ptr{UInt64}, Ptr{Cvoid}),
        h, pointer(P.Position), pointer(P.Velocity), pointer(P.Acceleration), pointer(P.Density), pointer(typ), pointer(P.ID),
        pointer(P.GroupMarker), B <: SimpleMDBC ? pointer(P.GhostPoints) : C_NULL))
    check(h, ccall((:sphmi_set_clock, LIB), Cint, (Ptr{Cvoid}, Int64, Float64), h, SimMetaData.Iteration, SimMetaData.TotalTime))
    for a in (P.Position, P.Velocity, P.Acceleration, P.Density, P.Pressure, P.ID, P.GroupMarker, P.Cells)
        pin(h, a)
    end
    B <: SimpleMDBC && pin(h, P.GhostPoints)
    # the columns the engine does not carry ride on the device as opaque rows (the arrays of the StructArray keep their addresses)
    columns = Any[]
    if get(ENV, "SPHMI_COLUMNS", "1") != "0"
        append!(columns, (P.GravityFactor, P.MotionLimiter, P.BoundaryBool, P.GhostNormals, P.ChunkID, P.Type))
        K <: StoreKernelOutput || append!(columns, (P.Kernel, P.KernelGradient))
    end
    colptrs = Ptr{Cvoid}[Ptr{Cvoid}(pointer(a)) for a in columns]
    if !isempty(columns)
        widths = Int32[Int32(sizeof(eltype(a))) for a in columns]
        GC.@preserve columns colptrs widths check(h, ccall((:sphmi_attach_columns, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Ptr{Cvoid}}, Ptr{Int32}),
                                                          h, Int32(length(columns)), pointer(colptrs), pointer(widths)))
        foreach(a -> pin(h, a), columns)
    end
    markers = group_force_markers()                # opt-in: nothing is recorded, and nothing more launched, without SPHMI_GROUP_FORCES
    if !isempty(markers)
        GC.@preserve markers check(h, ccall((:sphmi_group_forces_enable, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{UInt64}, Int64),
                                            h, Int32(length(markers)), pointer(markers), 1 << 20))
        GROUP_FORCES[P] = GroupForceSeries(markers, Int64[], Float64[], Float64[], Array{Float64,3}(undef, 3, length(markers), 0), 0)
    end
    points = probe_positions(D)                    # opt-in as well: SPHMI_PROBES
    if !isempty(points)
        m = size(points, 2)
        GC.@preserve points check(h, ccall((:sphmi_probes_enable, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64), h, Int32(m), pointer(points), 1 << 16))
        PROBES[P] = ProbeSeries(points, Int64[], Float64[], Float64[], zeros(Float64, m, 0), zeros(Int64, m, 0), zeros(Float64, m, 0), zeros(Float64, m, 0),
                                Array{Float64,3}(undef, 3, m, 0), 0)
    end
    mpoints = probe_positions(D, "SPHMI_PROBE_MOMENTS")      # opt-in as well: SPHMI_PROBE_MOMENTS, a point set of its own
    if !isempty(mpoints)
        m = size(mpoints, 2)
        GC.@preserve mpoints check(h, ccall((:sphmi_probe_moments_enable, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Int64), h, Int32(m), pointer(mpoints), 1 << 16))
        e3 = Array{Float64,3}(undef, 3, m, 0)
        PROBE_MOMENTS[P] = ProbeMomentSeries(mpoints, Int64[], Float64[], Float64[], zeros(Float64, m, 0), zeros(Int64, m, 0), zeros(Float64, m, 0), zeros(Float64, m, 0),
                                             e3, e3, Array{Float64,3}(undef, 6, m, 0), e3, e3, Array{Float64,4}(undef, 3, 3, m, 0), 0)
    end
    if budgets_wanted()                            # opt-in as well: SPHMI_BUDGETS
        check(h, ccall((:sphmi_budgets_enable, LIB), Cint, (Ptr{Cvoid}, Int64), h, 1 << 20))
        BUDGETS[P] = BudgetSeries(Int64[], Float64[], Float64[], Int64[], zeros(Float64, 3, 0), zeros(Float64, 3, 0), zeros(Float64, 3, 0), zeros(Float64, 3, 0),
                                  zeros(Float64, 3, 0), zeros(Float64, 6, 0), 0)
    end
    box_lo, box_hi = flow_boxes(D)                 # opt-in as well: SPHMI_FLOW_BOXES
    if !isempty(box_lo)
        m = size(box_lo, 2)
        GC.@preserve box_lo box_hi check(h, ccall((:sphmi_flow_enable, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float64}, Ptr{Float64}, Int64),
                                                  h, Int32(m), pointer(box_lo), pointer(box_hi), 1 << 20))
        FLOW[P] = FlowSeries(box_lo, box_hi, Int64[], Float64[], Float64[], zeros(Int64, m, 0), zeros(Float64, m, 0), Array{Float64,3}(undef, 3, m, 0),
                             zeros(Int64, m, 0), zeros(Int64, m, 0), 0)
    end
    mask = envelopes_mask()                        # opt-in as well: SPHMI_ENVELOPES
    if mask != 0
        envelopes_enable(h, mask)
        ENVELOPES[P] = Envelopes(mask, 0, 0.0, 0.0, 0.0, Float64[], Float64[], Float64[], Float64[], Float64[], Float64[], Float64[], Float64[])
    end
    lattice = maps_lattice(D)                      # opt-in as well: SPHMI_MAPS
    if lattice !== nothing
        maps_enable(h, lattice...)
        e = Float64[]
        MAPS[P] = Maps(lattice..., 0, 0.0, 0.0, 0.0, e, e, e, e, e, e, e, e, e, e, Int64[], e, e, e)
    end
    traced = tracer_spec(D)                        # opt-in as well: SPHMI_TRACERS
    if traced !== nothing
        tracers_enable(h, traced...)
        TRACERS[P] = TracerSeries(traced..., Int64[], Float64[], Float64[], Array{Float64,3}(undef, 8, length(traced[1]), 0),
                                  Array{Float64,3}(undef, 10, size(traced[2], 2), 0), zeros(Float64, 3, size(traced[2], 2)), 0)
    end
    return Session(h, Vector{Int64}(undef, N), zeros(8), zeros(Int64, 8), Vector{Int}(undef, N), Vector{Int64}(undef, SimMetaData.ExportGridCells ? N * D : 0),
                   columns, colptrs)
    catch
        ccall((:sphmi_destroy, LIB), Cint, (Ptr{Cvoid},), h)
        rethrow()
    end
end

# The engine's phases under the reference's own TimerOutputs labels (src/SPHCellList.jl:748-798: "01 Update TimeStep", "02a Actual
# Calculate IndexCounter", "04 Apply MDBC before Half TimeStep", "05 First NeighborLoop", "08 Second NeighborLoop"), nested under
# "00 SimulationLoop" (:883) like the reference's: a section is opened empty, then credited with the DEVICE seconds and calls the
# engine measured since the previous interval (`accumulated_data` is TimerOutputs' own field: ncalls, time in ns).
function forward_timers!(to::TimerOutput, s::Session)
    names = Vector{Cstring}(undef, 8); secs = zeros(8); calls = zeros(Int64, 8); n = Ref{Int32}(0)
    check(s.h, ccall((:sphmi_timers, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Cstring}, Ptr{Float64}, Ptr{Int64}, Ref{Int32}), s.h, 8, names, secs, calls, n))
    for k in 1:min(Int(n[]), 5)
        label = unsafe_string(names[k])
        @timeit to label nothing
        d = (isempty(to.timer_stack) ? to : to.timer_stack[end])[label].accumulated_data
        d.time += round(Int64, (secs[k] - s.secs[k]) * 1e9); d.ncalls += calls[k] - s.calls[k] - 1
    end
    s.secs .= secs; s.calls .= calls
end

# the reference's sort! permutes every column (src/SPHCellList.jl:142): the ones the engine does not carry follow by gather
permute_column!(a::AbstractVector, perm) = (a .= a[perm]; nothing)

# One output interval on the device: the contract of src/SPHCellList.jl:727-805 — advance until TotalTime > next output
# time, leave the state in SimParticles (cell-sorted, every field permuted alike) and the counters in SimMetaData.
function SimulationLoop(SimDensityDiffusion::BuiltinDDT, SimViscosity::BuiltinViscosity, SimKernel,
                        SimMetaData::SimulationMetaData{D,T,S,K,B,L}, SimConstants, SimParticles, Stencil, ParticleRanges,
                        UniqueCells, CellDict, SortingScratchSpace, SimThreadedArrays, dρdtI, Velocityₙ⁺, Positionₙ⁺, ρₙ⁺,
                        ∇Cᵢ, ∇◌rᵢ, MotionDefinition) where {D,T,S,K,B,L}
    P = SimParticles
    s = get!(() -> open_session(SimDensityDiffusion, SimViscosity, SimKernel, SimMetaData, SimConstants, P, MotionDefinition), SESSIONS, P)
    h = s.h
    prog = SphmiProgress()
    check(h, ccall((:sphmi_advance, LIB), Cint, (Ptr{Cvoid}, Float64, Int64, Ref{SphmiProgress}), h, Float64(next_output_time(SimMetaData)), -1, prog))
    SimMetaData.Iteration, SimMetaData.CurrentTimeStep, SimMetaData.TotalTime = prog.iteration, T(prog.last_dt), T(prog.total_time)
    SimMetaData.IndexCounter = prog.index_counter
    forward_timers!(SimMetaData.HourGlass, s)
    haskey(GROUP_FORCES, P) && read_group_forces!(h, GROUP_FORCES[P])
    haskey(PROBES, P) && read_probes!(h, PROBES[P])
    haskey(PROBE_MOMENTS, P) && read_probe_moments!(h, PROBE_MOMENTS[P])
    haskey(BUDGETS, P) && read_budgets!(h, BUDGETS[P])
    haskey(FLOW, P) && read_flow!(h, FLOW[P])
    haskey(ENVELOPES, P) && read_envelopes!(h, ENVELOPES[P], length(P))
    haskey(MAPS, P) && read_maps!(h, MAPS[P])
    haskey(TRACERS, P) && read_tracers!(h, TRACERS[P])
    GC.@preserve P s begin
        # the carried fields: snapshot on the device, copies on a second stream, straight into the StructArray's columns
        # (Cells: a Vector{CartesianIndex{D}} is N·D Int64; Type is a per-particle constant and follows the gather below)
        check(h, ccall((:sphmi_download_begin, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ptr{UInt8}, Ptr{UInt64}, Ptr{Cvoid}, Ptr{Int64}),
            h, pointer(P.Position), pointer(P.Velocity), pointer(P.Acceleration), pointer(P.Density), pointer(P.Pressure),
            pointer(P.ID), C_NULL, pointer(P.GroupMarker), B <: SimpleMDBC ? pointer(P.GhostPoints) : C_NULL,
            Ptr{Int64}(pointer(P.Cells))))
        if !isempty(s.columns)
            # the passive columns: a second snapshot of the same rows (no step in between), copied like the fields
            check(h, ccall((:sphmi_download_columns_begin, LIB), Cint, (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}), h, pointer(s.colptrs)))
        else
            # SPHMI_COLUMNS=0 — while the copies are in flight: the sort as a permutation, and one gather per passive column
            check(h, ccall((:sphmi_download_permutation, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), h, pointer(s.prev_row)))
            s.perm .= s.prev_row .+ 1
            for col in (P.Type, P.GravityFactor, P.MotionLimiter, P.BoundaryBool, P.GhostNormals, P.ChunkID)
                permute_column!(col, s.perm)
            end
            K <: StoreKernelOutput || (permute_column!(P.Kernel, s.perm); permute_column!(P.KernelGradient, s.perm))
        end
        if K <: StoreKernelOutput
            check(h, ccall((:sphmi_download_kernel_output, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}), h, pointer(P.Kernel), pointer(P.KernelGradient)))
        end
        if SimMetaData.ExportGridCells     # UniqueCells[2:IndexCounter] for save_grid (:890-893); slot 1 is the reference's dummy entry (:145-147)
            nref = Ref{Int64}(0)
            check(h, ccall((:sphmi_unique_cells, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Int64, Ref{Int64}), h, pointer(s.ucells), length(P), nref))
            @inbounds for k in 1:min(Int(nref[]), length(UniqueCells) - 1)
                UniqueCells[k + 1] = CartesianIndex(ntuple(d -> Int(s.ucells[(k - 1) * D + d]), D))
            end
        end
        check(h, ccall((:sphmi_download_end, LIB), Cint, (Ptr{Cvoid},), h))
    end
    if SimMetaData.TotalTime > SimMetaData.SimulationTime                              # last interval (:909): release the GPUs
        ccall((:sphmi_destroy, LIB), Cint, (Ptr{Cvoid},), h); delete!(SESSIONS, P)
    end
    return nothing
end

end # module
