"""``RunSimulation`` — host-side mirror of the reference's driver loop around the hot path.

Restates the bookkeeping of /root/reference/src/SPHCellList.jl:808-930 that surrounds
``SimulationLoop``: load mDBC normals (:827), output counter starts at 1 (:849), one engine
``advance`` per output interval (:883) with ``next_output_time`` (:687-698), stop when
``TotalTime > SimulationTime`` (:909).  VTKHDF output, logging and ParaView glue are out of scope
(SURVEY.md §2 rows 11-13); ``on_output`` receives the particles at every output time instead.
"""
from __future__ import annotations

import copy
import os
from typing import Callable, List, Optional

import numpy as np

from ._abi import Backend, make_config
from .config import (SimulationConstants, SimulationMetaData, SPHDensityDiffusion, SPHKernelInstance,
                     SPHViscosity, next_output_time)
from .budgets import empty_budgets
from .flow import empty_flow
from .probes import empty_probe_moments
from .engine import Engine
from .preprocess import LoadMDBCNormals, SimParticles

# Fields of the StructArray the engine does not carry (src/PreProcess.jl:114): the reference's sort! (src/SPHCellList.jl:142)
# permutes them with everything else, so after a download they follow through the engine's own permutation
# (sphmi_download_permutation) — one gather per field, no sort on the host.  Backends with sphmi_attach_columns keep them on
# the device instead and deliver them with every output (SPHMI_COLUMNS=0: the host gathers, for A/B runs).
PASSIVE_FIELDS = ("ChunkID", "GravityFactor", "MotionLimiter", "BoundaryBool", "GhostNormals")


def permute_passive_fields(particles: SimParticles, prev_row, kernel_output: bool = False) -> None:
    """Row i of the downloaded arrays was row prev_row[i] at the previous call: bring the passive fields along.  Kernel /
    KernelGradient are passive too unless the handle stores them (StoreKernelOutput: they are downloaded instead)."""
    names = PASSIVE_FIELDS + (() if kernel_output else ("Kernel", "KernelGradient"))
    for k in names:
        a = getattr(particles, k)
        a[...] = np.take(a, prev_row, axis=0)          # (take: 6 ms for a million rows × 3 where a[prev_row] needs 38)


def RunSimulation(*, SimGeometry=None, SimMetaData: SimulationMetaData, SimConstants: SimulationConstants,
                  SimKernel: SPHKernelInstance, SimLogger=None, SimParticles: SimParticles,
                  SimViscosity: SPHViscosity, SimDensityDiffusion: SPHDensityDiffusion,
                  ParticleNormalsPath: Optional[str] = None,
                  on_output: Optional[Callable[[SimulationMetaData, SimParticles], None]] = None,
                  device_float_bytes: int = 0, device: int = 0, backend_factory=None,
                  async_output: bool = False, group_forces=None, probes=None, field_grid=None,
                  particle_fields=None, budgets: bool = False, neighbor_list: bool = False, isosurface=None, components=None,
                  flow_boxes=None, envelopes=None, maps=None, tracers=None, sample_points=None,
                  sample_point_gradients=None, rays=None, output_select=None, sample_point_moments=None,
                  probe_moments=None) -> List[float]:
    """Same keyword signature as the reference (src/SPHCellList.jl:808-817); returns the list of
    time steps the reference collects in ``TimeSteps`` (:823,:884).  ``SimParticles`` is updated in
    place at every output time, in the engine's cell-sorted order, as the reference's is.

    ``group_forces=[markers]``: the force on those particle groups is recorded on the device at every step
    (``Backend.group_forces_enable``) and ``on_output`` is called with a third argument, the samples of the interval that ends
    at this output, ``(iteration[n], time[n], dt[n], F[n, len(markers), 3])`` (empty arrays at the first call).  ``None``
    (default): nothing is recorded and the callback keeps its two arguments.

    ``probes=positions`` ([n, dims]): pressure, density and velocity are sampled at those fixed points on the device at every
    step (``Backend.probes_enable``; ``sphexample_amd.probes`` builds gauge columns and reads water levels off them) and
    ``on_output`` receives the samples of the interval as one more argument, the dict of ``Backend.probes_read`` — behind the
    group forces when both are asked for.

    ``field_grid=(origin, spacing, counts)``: at every output the same sums are sampled on that regular lattice
    (``Backend.sample_grid``; ``sphexample_amd.fields`` forms the node coordinates and reads a surface height off the
    result) and ``on_output`` receives the dict of fields as one more argument, behind group forces and probes when those
    are on — ``None`` at the first call, which precedes the first step.  ``None`` (default): nothing is sampled.

    ``particle_fields=(names…)``: at every output the differential fields of ``Backend.particle_fields`` — ``"count"``,
    ``"shepard"``, ``"normal"``, ``"div_r"``, ``"div_v"``, ``"vorticity"`` — are evaluated at the particles and ``on_output``
    receives the dict as one more argument, behind group forces, probes and the field grid when those are on (``None`` at the
    first call).  It is taken at the same point as the snapshot: row i is particle i of that output
    (``sphexample_amd.fields.free_surface_mask`` reads a free surface off ``div_r``).  ``None`` (default): nothing is evaluated
    and the callback keeps its arguments.

    ``neighbor_list=True``: at every output the CSR neighbour list of ``Backend.neighbor_list`` is built on the device and
    ``on_output`` receives ``(offsets, neighbors)`` as one more argument, behind the differential fields and before the budgets
    (``None`` at the first call).  It is taken at the same point as the snapshot, with no step between it and the download: row i
    is particle i of that output (``sphexample_amd.neighbors`` forms pair sums from it).  ``False`` (default): nothing is built
    and the callback keeps its arguments.

    ``isosurface=(origin, spacing, counts[, level])``: at every output the free surface is extracted on the device as a mesh
    (``Backend.isosurface`` on that lattice, level 0.5 unless given; ``sphexample_amd.isosurface`` measures it) and ``on_output``
    receives ``(vertices, elements)`` as one more argument, behind the neighbour list and before the budgets (``None`` at the
    first call), the way ``field_grid=`` hands over its fields.  ``None`` (default): nothing is extracted.

    ``components=True | link | (link, types)``: at every output the connected bodies of the fluid are labelled on the device
    (``Backend.components``: rows linked within `link`, H unless given, among the rows of `types`, the fluid unless given;
    ``sphexample_amd.components`` finds the main body and tabulates the droplets) and ``on_output`` receives the dict of
    ``label``, ``first_row``, ``count`` and ``box`` as one more argument, behind the mesh and before the budgets (``None`` at the
    first call).  Row i is particle i of that output.  ``None`` or ``False`` (default): nothing is built and the callback keeps
    its arguments.

    ``budgets=True``: the energy, momentum and extent budgets of the fluid are recorded on the device at every step
    (``Backend.budgets_enable``; ``sphexample_amd.budgets`` adds up a total energy and reads a wave front off the box) and
    ``on_output`` receives the samples of the interval, the dict of ``Backend.budgets_read``, as its last argument (empty
    arrays at the first call).  ``False`` (default): nothing is recorded and the callback keeps its arguments.

    ``flow_boxes=[(lo, hi), …]``: the flow through those half-open control boxes (``lo <= x < hi`` per axis, ``dims`` bounds each,
    ``±inf`` allowed; ``sphexample_amd.flow.strips`` tiles an axis) is recorded on the device at every step
    (``Backend.flow_enable``; ``sphexample_amd.flow`` forms discharges and cumulative counts) and ``on_output`` receives the
    samples of the interval, the dict of ``Backend.flow_read``, as one more argument behind the budgets (empty arrays at the
    first call).  ``None`` (default): nothing is recorded and the callback keeps its arguments.

    ``envelopes=True | types``: what every particle of `types` (the fluid for ``True``; ``"Fluid"``, ``"Fixed"``, ``"Moving"`` or a
    tuple of them) experiences is accumulated on the device at every step (``Backend.envelopes_enable``: peak pressure and its
    time, impulse, time under load, largest speed, arrival time; ``sphexample_amd.envelopes`` forms means and an arrival map) and
    ``on_output`` receives the dict of ``Backend.envelopes_read`` as its last argument, the way ``particle_fields=`` hands over its
    fields (``None`` at the first call).  The envelopes keep growing over the whole run; row i is particle i of that output.
    ``None`` or ``False`` (default): nothing is accumulated and the callback keeps its arguments.

    ``maps=(origin, spacing, counts[, up_axis])``: what every bin of that lattice experiences is accumulated on the device at every
    step (``Backend.maps_enable``: crest and its time, arrival time, wet duration, fill, flux, the largest bin-mean speed;
    ``sphexample_amd.maps`` forms depths, mean velocities and an arrival map) and ``on_output`` receives the dict of
    ``Backend.maps_read`` as its last argument, behind the envelopes (``None`` at the first call).  The maps keep growing over the
    whole run.  ``None`` (default): nothing is accumulated and the callback keeps its arguments.

    ``tracers=dict(particles=rows, drifters=points, min_weight=0.5)``: the rows `particles` of `SimParticles` are followed and
    the massless points `drifters` advected with the flow on the device at every step (``Backend.tracers_enable``;
    ``sphexample_amd.tracers.pathlines`` joins the intervals into one array of positions) and ``on_output`` receives the steps of
    the interval, the dict of ``Backend.tracers_read``, as its last argument, behind the maps (``None`` at the first call).  Either
    key may be missing.  ``None`` (default): nothing is followed and the callback keeps its arguments.

    ``sample_points=positions`` ([n, dims]): at every output the sums of the field grid are sampled at those arbitrary points
    (``Backend.sample_points``; ``sphexample_amd.fields`` forms panel centroids and integrates a surface load) and ``on_output``
    receives the dict — ``weight``, ``count``, ``pressure``, ``density`` [n], ``velocity`` [n, 3] — as its last argument, behind the
    tracers (``None`` at the first call, which precedes the first step).  ``None`` (default): nothing is sampled and the callback
    keeps its arguments.

    ``sample_point_gradients=positions`` ([n, dims]): at every output the raw kernel and gradient sums are sampled at those points
    (``Backend.sample_point_gradients``; ``sphexample_amd.fields`` turns them into the velocity gradient, vorticity, divergence,
    strain rate, pressure gradient and free-surface normal) and ``on_output`` receives the dict as its last argument, behind
    ``sample_points`` (``None`` at the first call).  ``None`` (default): nothing is sampled and the callback keeps its arguments.

    ``rays=dict(origins=…, directions=…, t_end=…, …)``: at every output those rays are cast through the fluid (the keywords of
    ``Backend.cast_rays``; ``sphexample_amd.rays`` builds gauges and depth images on it) and ``on_output`` receives the dict —
    ``status``, ``interval``, ``bracket``, ``point`` and the raw sums at the hit — as its last argument, behind
    ``sample_point_gradients`` (``None`` at the first call).  ``None`` (default): nothing is cast and the callback keeps its
    arguments.

    ``output_select=spec`` (a ``sphexample_amd.selection.Selection``, or ``(spec, fields)`` to name the fields wanted): at every
    output the rows `spec` selects are compacted on the device (``Backend.select``; ``sphexample_amd.selection`` builds slabs,
    decimations and masks) and ``on_output`` receives ``(rows, dict of arrays)`` as its last argument, behind the rays.  It is taken
    at the same point as the snapshot, with no step between it and the download: ``rows`` index the particles of that output and
    every array equals that field's ``[rows]``.  A selection needs no executed step, so the first call receives one too, of the
    particles as uploaded.  ``None`` (default): nothing is selected and the callback keeps its arguments.

    ``sample_point_moments=positions`` ([n, dims]): at every output the raw kernel sums and their first and second moments are
    sampled at those points (``Backend.sample_point_moments``; ``sphexample_amd.fields.linear_fit`` turns them into values and
    gradients that are exact for a linear field however one-sided the support — sensors on a wall, on the bed, at the free surface)
    and ``on_output`` receives the dict as its last argument, behind ``output_select`` (``None`` at the first call).  ``None``
    (default): nothing is sampled and the callback keeps its arguments.

    ``probe_moments=positions`` ([n, dims]): the same moment sums are recorded at those fixed points on the device at EVERY step
    (``Backend.probe_moments_enable``; ``sphexample_amd.probes.fit_series`` turns a record into the fitted signal of every probe at
    every step) and ``on_output`` receives the samples of the interval, the dict of ``Backend.probe_moments_read``, as its last
    argument, behind ``sample_point_moments`` — as ``probes=`` hands over its samples (empty arrays at the first call).  ``None``
    (default): nothing is recorded and the callback keeps its arguments."""
    if SimMetaData.BMode.__name__ == "SimpleMDBC":
        LoadMDBCNormals(SimParticles, ParticleNormalsPath)                       # :827
    host_bytes = SimParticles.Position.dtype.itemsize
    cfg = make_config(len(SimParticles), SimConstants, SimKernel, SimMetaData, SimViscosity,
                      SimDensityDiffusion, device_float_bytes=device_float_bytes,
                      host_float_bytes=host_bytes, device=device)
    eng = (backend_factory or Engine)(cfg)
    eng.upload_particles(SimParticles)
    eng.set_motions(SimGeometry)                      # MotionDefinition, src/SPHCellList.jl:846-850
    kout = SimMetaData.KMode.__name__ == "StoreKernelOutput"
    # the fields the engine does not carry: on the device with the particles when the backend can hold them
    columns = None
    if getattr(eng, "has_columns", lambda: False)() and os.environ.get("SPHMI_COLUMNS", "1") != "0":
        columns = [getattr(SimParticles, k) for k in PASSIVE_FIELDS + (() if kout else ("Kernel", "KernelGradient"))]
        if all(isinstance(a, np.ndarray) and a.flags.c_contiguous and len(a) == len(SimParticles) for a in columns):
            eng.attach_columns(columns)
        else:
            columns = None                             # a field in another layout: the host gathers take any
    if on_output:
        eng.pin(SimParticles)                          # the same arrays receive every output
        if columns:
            eng.pin(columns)
    eng.set_clock(SimMetaData.Iteration, SimMetaData.TotalTime)
    time_steps: List[float] = []
    SimMetaData.OutputIterationCounter = 1                                       # :849
    dims = SimMetaData.Dimensions
    cloud = lambda v: np.ascontiguousarray(v, dtype=np.float64).reshape(-1, dims)            # noqa: E731
    chosen = lambda v: None if v is False else v                                             # noqa: E731
    series = Backend.empty_series

    def boxes(v):
        if len(v) == 0:
            raise ValueError("RunSimulation: flow_boxes holds no box (pass None to record nothing)")
        return [(np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)) for lo, hi in v]

    # What the callback receives behind the particles, in this order.  Per row: the keyword's value (None: off), what makes its
    # normal form `a` of it, the enable call, the first value — handed over before the first step — and the reader of every later
    # output.  No enable: nothing is recorded between the outputs, the reader evaluates the state of its output (no step lies
    # between it and the download).  No first value: None at the first call.
    table = (
        (group_forces, lambda v: [int(m) for m in v], lambda a: eng.group_forces_enable(a, capacity=1 << 20),
         lambda a: tuple(series(Backend.GROUP_FORCE_FIELDS, len(a)).values()), lambda a: eng.group_forces_read()),
        (probes, cloud, lambda a: eng.probes_enable(a, capacity=1 << 16),
         lambda a: series(Backend.PROBE_FIELDS, len(a)), lambda a: eng.probes_read()),
        (field_grid, tuple, None, None, lambda a: eng.sample_grid(*a)),
        (particle_fields, tuple, None, None, lambda a: eng.particle_fields(a)),
        (neighbor_list or None, bool, None, None, lambda a: eng.neighbor_list()),
        (isosurface, tuple, None, None, lambda a: eng.isosurface(*a)),
        (chosen(components), lambda v: () if v is True else tuple(v) if isinstance(v, (tuple, list)) else (v,), None, None,
         lambda a: eng.components(*a)),
        (budgets or None, bool, lambda a: eng.budgets_enable(capacity=1 << 20), lambda a: empty_budgets(), lambda a: eng.budgets_read()),
        (flow_boxes, boxes, lambda a: eng.flow_enable([lo for lo, _ in a], [hi for _, hi in a], capacity=1 << 20),
         lambda a: empty_flow(len(a)), lambda a: eng.flow_read()),
        (chosen(envelopes), lambda v: ("Fluid",) if v is True else v, lambda a: eng.envelopes_enable(a), None, lambda a: eng.envelopes_read()),
        (maps, tuple, lambda a: eng.maps_enable(*a), None, lambda a: eng.maps_read()),
        (tracers, dict, lambda a: eng.tracers_enable(capacity=1 << 16, **a), None, lambda a: eng.tracers_read()),
        (sample_points, cloud, None, None, lambda a: eng.sample_points(a)),
        (sample_point_gradients, cloud, None, None, lambda a: eng.sample_point_gradients(a)),
        (rays, dict, None, None, lambda a: eng.cast_rays(**a)),
        (output_select, lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,), None, lambda a: eng.select(*a), lambda a: eng.select(*a)),
        (sample_point_moments, cloud, None, None, lambda a: eng.sample_point_moments(a)),
        (probe_moments, cloud, lambda a: eng.probe_moments_enable(a, capacity=1 << 16),
         lambda a: empty_probe_moments(len(a), dims, float(SimKernel.h)), lambda a: eng.probe_moments_read()),
    )
    extras = []          # per output: what the callback receives behind the particles — a list of (first value, reader)
    for value, normal, enable, first, read in table:
        if value is None:
            continue
        a = normal(value)
        if enable:
            enable(a)
        extras.append((first(a) if first else None, lambda read=read, a=a: read(a)))
    none_yet = tuple(first for first, _ in extras)
    emit = lambda meta, samples: on_output(meta, SimParticles, *samples)         # noqa: E731
    if on_output:
        emit(SimMetaData, none_yet)                                              # :850

    def finish_output(begin_only: bool = False):
        """The fields the engine does not carry follow the sort; a StoreKernelOutput handle hands over Kernel / KernelGradient."""
        if columns:
            (eng.download_columns_begin if begin_only else eng.download_columns)(columns)
        elif eng._has("download_permutation"):
            permute_passive_fields(SimParticles, eng.download_permutation(), kernel_output=kout)
        if kout:
            SimParticles.Kernel[...], SimParticles.KernelGradient[...] = eng.kernel_output()

    pending = None       # async_output: metadata of the snapshot whose copies are in flight
    while True:                                                                  # :881
        prog = eng.advance(next_output_time(SimMetaData))                        # :883
        SimMetaData.Iteration = prog.iteration
        SimMetaData.CurrentTimeStep = prog.last_dt
        SimMetaData.TotalTime = prog.total_time
        SimMetaData.IndexCounter = prog.index_counter
        time_steps.append(prog.last_dt)                                          # :884
        SimMetaData.OutputIterationCounter += 1                                  # :888
        done = SimMetaData.TotalTime > SimMetaData.SimulationTime               # :909
        samples = tuple(read() for _, read in extras)                            # the steps of this interval
        if on_output and async_output:
            # The copies of snapshot k run while interval k+1 is computed: the callback for k is made after the
            # NEXT advance, with the metadata captured at the snapshot.
            if pending is not None:
                eng.download_end()
                emit(*pending)
            eng.download_into_begin(SimParticles)
            finish_output(begin_only=True)     # (attached columns: a second snapshot in flight; otherwise host-side gathers that overlap the copies)
            pending = (copy.copy(SimMetaData), samples)
            if done:
                eng.download_end()
                emit(*pending)
                break
            continue
        if on_output:
            eng.download_into(SimParticles)
            finish_output()
            emit(SimMetaData, samples)                                           # :891-894
        if done:
            if not on_output:
                eng.download_into(SimParticles)
                finish_output()
            break
    eng.unpin()
    eng.close()
    return time_steps
