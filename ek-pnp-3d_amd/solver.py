"""ctypes binding of libekpnp.so (include/ekpnp.h).

`Solver` mirrors the reference's host step API one to one:

    reference (LBM.h)                      here
    -------------------------------------  ------------------------------
    initialization(r,c,cn,fi,u,v,w,...)    Solver.initialization()
    init_equilibrium(f0,f1,...,temp)       Solver.init_equilibrium()
    stream_collide_save(f0,...,t,f0bc)     Solver.stream_collide_save(t)
    fast_Poisson(charge,chargen,kx,ky,kz)  Solver.fast_Poisson()
    main.cu:189-200 loop body x n          Solver.step(n)

Errors: the reference prints and exit()s (LBM.cu:35-53); here every non-zero status of the
C ABI raises EkpnpError carrying ekpnp_last_error().
"""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBNAME = "libekpnp.so"

FIELDS = ["rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T"]
FIELD_ID = {n: i for i, n in enumerate(FIELDS)}
# the EKPNP_NPROFILES plane sums of ekpnp_plane_sums, in id order (include/ekpnp.h: EKPNP_PROF_*); q stands for c - cn
PROFILE_NAMES = FIELDS + ["ux_ux", "uy_uy", "uz_uz", "c_c", "cn_cn", "T_T", "uz_T", "uz_c", "uz_cn", "q_Ex", "q_Ez", "ux_uz", "q_q"]
PROFILE_ID = {n: i for i, n in enumerate(PROFILE_NAMES)}
# the EKPNP_NMONITORS scalars of a monitor row, in id order (include/ekpnp.h: EKPNP_MON_*); q stands for c - cn
MONITOR_NAMES = ["current_top", "current_bottom", "dTdz_bottom", "dTdz_top", "uz_max", "u_u", "q", "q_q", "uz_T", "rho_dev", "nonfinite"]
MONITOR_ID = {n: i for i, n in enumerate(MONITOR_NAMES)}


class EkpnpError(RuntimeError):
    pass


class SnapshotSpec(C.Structure):
    """Mirror of `ekpnp_snapshot_spec` (include/ekpnp.h): field bit mask (0 = all eleven) and the coarsening cx, cy, cz."""

    _fields_ = [("fields", C.c_uint32), ("cx", C.c_int32), ("cy", C.c_int32), ("cz", C.c_int32)]


def snapshot_spec(fields=None, coarsen=(1, 1, 1)) -> SnapshotSpec:
    """fields: None (all eleven), a bit mask over the field ids, or names; the output keeps ascending id order"""
    if fields is None:
        mask = 0
    elif isinstance(fields, int):
        mask = fields
    else:
        mask = 0
        for n in fields:
            mask |= 1 << FIELD_ID[n]
        if mask == 0:
            raise ValueError("snapshot: no field selected")
    cx, cy, cz = (int(v) for v in coarsen)
    return SnapshotSpec(mask, cx, cy, cz)


class MonitorSpec(C.Structure):
    """Mirror of `ekpnp_monitor_spec` (include/ekpnp.h): quantity bit mask (0 = all eleven), a row every `every` steps, ring rows."""

    _fields_ = [("quantities", C.c_uint32), ("every", C.c_int32), ("capacity", C.c_int32)]


def monitor_mask(quantities=None) -> int:
    """None (all eleven), a bit mask over the monitor ids, or names"""
    if quantities is None:
        return 0
    if isinstance(quantities, int):
        return quantities
    mask = 0
    for n in quantities:
        mask |= 1 << (MONITOR_ID[n] if isinstance(n, str) else int(n))
    if mask == 0:
        raise ValueError("monitor: no quantity selected")
    return mask


def monitor_spec_check(quantities=None, every: int = 1, capacity: int = 1) -> MonitorSpec:
    """the spec, or EkpnpError with the library's message (ekpnp_monitor_spec_check: host arithmetic, no device)"""
    L = load_library()
    spec = MonitorSpec(monitor_mask(quantities), int(every), int(capacity))
    rc = L.ekpnp_monitor_spec_check(C.byref(spec))
    if rc:
        raise EkpnpError(f"ekpnp_monitor_spec_check -> status {rc}: {L.ekpnp_last_error(None).decode()}")
    return spec


SEED_PATTERNS = {"none": 0, "noise": 0, "rolls": 1, "squares": 2, "hexagons": 3}  # include/ekpnp.h: EKPNP_SEED_*
MAX_MODES = 16


class SeedSpec(C.Structure):
    """Mirror of `ekpnp_seed_spec` (include/ekpnp.h): which fields, which pattern with how many periods across nx and ny,
    relative or absolute, the noise seed, the pattern's amplitude A and the noise's B."""

    _fields_ = [("fields", C.c_uint32), ("pattern", C.c_int32), ("mx", C.c_int32), ("my", C.c_int32), ("relative", C.c_int32),
                ("reserved", C.c_int32), ("seed", C.c_uint64), ("amplitude", C.c_double), ("noise", C.c_double)]


def seed_spec(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude: float = 1e-3, noise: float = 0.0, relative: bool = True,
              seed: int = 1) -> SeedSpec:
    """fields: a bit mask over the field ids or names out of rho, c, cn, ux, uy, uz, T; pattern: a name of SEED_PATTERNS or its id"""
    if isinstance(fields, int):
        mask = fields
    else:
        mask = 0
        for n in fields:
            mask |= 1 << (FIELD_ID[n] if isinstance(n, str) else int(n))
    pat = SEED_PATTERNS[pattern] if isinstance(pattern, str) else int(pattern)
    return SeedSpec(mask, pat, int(modes[0]), int(modes[1]), int(relative), 0, int(seed), float(amplitude), float(noise))


class ModesSpec(C.Structure):
    """Mirror of `ekpnp_modes_spec` (include/ekpnp.h): the field and up to MAX_MODES x-y modes (m, n) to project it onto."""

    _fields_ = [("field_id", C.c_int32), ("nmodes", C.c_int32), ("m", C.c_int32 * MAX_MODES), ("n", C.c_int32 * MAX_MODES)]


def modes_spec(field="uz", modes=((1, 1),)) -> ModesSpec:
    """field: a name or an id; modes: pairs (m, n) with 0 <= m <= nx/2 and -(ny-1)/2 <= n <= ny/2"""
    modes = [(int(m), int(n)) for m, n in modes]
    spec = ModesSpec()
    spec.field_id = FIELD_ID[field] if isinstance(field, str) else int(field)
    spec.nmodes = len(modes)
    for j, (m, n) in enumerate(modes[:MAX_MODES]):
        spec.m[j], spec.n[j] = m, n
    return spec


def _as_modes_spec(field, modes) -> ModesSpec:
    return field if isinstance(field, ModesSpec) else modes_spec(field, modes)


def seed_spec_check(p: "Params", spec: SeedSpec) -> SeedSpec:
    """the spec, or EkpnpError with the library's message (ekpnp_seed_spec_check: host arithmetic, no device)"""
    L = load_library()
    rc = L.ekpnp_seed_spec_check(C.byref(p), C.byref(spec))
    if rc:
        raise EkpnpError(f"ekpnp_seed_spec_check -> status {rc}: {L.ekpnp_last_error(None).decode()}")
    return spec


def modes_spec_check(p: "Params", spec: ModesSpec) -> ModesSpec:
    """the spec, or EkpnpError with the library's message (ekpnp_modes_spec_check: host arithmetic, no device)"""
    L = load_library()
    rc = L.ekpnp_modes_spec_check(C.byref(p), C.byref(spec))
    if rc:
        raise EkpnpError(f"ekpnp_modes_spec_check -> status {rc}: {L.ekpnp_last_error(None).decode()}")
    return spec


def seed_uniform(seed: int, node: int, field) -> float:
    """the noise of (seed, global node index, field): Philox4x32-10, exact in [-1, 1) (ekpnp_seed_uniform, host only)"""
    fid = FIELD_ID[field] if isinstance(field, str) else int(field)
    return float(load_library().ekpnp_seed_uniform(int(seed), int(node), fid))


def seed_host(p: "Params", spec: SeedSpec, field, planes, z0: int = 0) -> np.ndarray:
    """THE definition of a seed, on the host: a seeded copy of `planes` ([nz_local][ny][nx], the global planes z0 ..) of `field`
    (ekpnp_seed_host; Solver.seed leaves the same bits in the device arrays)"""
    L = load_library()
    fid = FIELD_ID[field] if isinstance(field, str) else int(field)
    a = np.array(planes, dtype=np.float64, order="C", copy=True)
    if a.ndim != 3 or a.shape[1:] != (p.ny, p.nx):
        raise ValueError(f"planes must be [nz_local][{p.ny}][{p.nx}], got {a.shape}")
    rc = L.ekpnp_seed_host(C.byref(p), C.byref(spec), fid, int(z0), int(a.shape[0]), a.ctypes.data_as(C.c_void_p))
    if rc:
        raise EkpnpError(f"ekpnp_seed_host -> status {rc}: {L.ekpnp_last_error(None).decode()}")
    return a


MAX_SPECTRUM_PLANES = 16


class SpectrumSpec(C.Structure):
    """Mirror of `ekpnp_spectrum_spec` (include/ekpnp.h): the field and up to MAX_SPECTRUM_PLANES global z planes (0: every plane)."""

    _fields_ = [("field_id", C.c_int32), ("nplanes", C.c_int32), ("z", C.c_int32 * MAX_SPECTRUM_PLANES)]


def spectrum_spec(field="uz", planes=None) -> SpectrumSpec:
    """field: a name or an id; planes: None (every plane of the context, synchronous calls only) or global z indices, strictly ascending"""
    spec = SpectrumSpec()
    spec.field_id = FIELD_ID[field] if isinstance(field, str) else int(field)
    planes = [] if planes is None else [int(z) for z in planes]
    spec.nplanes = len(planes)
    for j, z in enumerate(planes[:MAX_SPECTRUM_PLANES]):
        spec.z[j] = z
    return spec


def _as_spectrum_spec(field, planes) -> SpectrumSpec:
    return field if isinstance(field, SpectrumSpec) else spectrum_spec(field, planes)


def spectrum_spec_check(p: "Params", spec: SpectrumSpec) -> SpectrumSpec:
    """the spec, or EkpnpError with the library's message (ekpnp_spectrum_spec_check: host arithmetic, no device)"""
    L = load_library()
    rc = L.ekpnp_spectrum_spec_check(C.byref(p), C.byref(spec))
    if rc:
        raise EkpnpError(f"ekpnp_spectrum_spec_check -> status {rc}: {L.ekpnp_last_error(None).decode()}")
    return spec


def spectrum_shells(p: "Params"):
    """(shell_of[ny][nx/2 + 1], count[nshell]): the shell of every mode of rfft2's layout and the number of modes per shell - THE
    binning of the shell spectra (ekpnp_spectrum_shells: host arithmetic, no device)"""
    L = load_library()
    n = C.c_int()
    rc = L.ekpnp_spectrum_shell_count(C.byref(p), C.byref(n))
    if rc:
        raise EkpnpError(f"ekpnp_spectrum_shell_count -> status {rc}: {L.ekpnp_last_error(None).decode()}")
    shell_of = np.zeros((p.ny, p.nx // 2 + 1), dtype=np.int32)
    count = np.zeros(n.value, dtype=np.int32)
    rc = L.ekpnp_spectrum_shells(C.byref(p), shell_of.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p))
    if rc:
        raise EkpnpError(f"ekpnp_spectrum_shells -> status {rc}: {L.ekpnp_last_error(None).decode()}")
    return shell_of, count


HIST_Q = 11  # include/ekpnp.h: EKPNP_HIST_Q, the charge density c - cn as a histogram value
HIST_MAX_BINS = 4096
HIST_VALUES = FIELDS + ["q"]
HIST_VALUE_ID = {n: i for i, n in enumerate(HIST_VALUES)}


class HistAxis(C.Structure):
    """Mirror of `ekpnp_hist_axis` (include/ekpnp.h): the value (a field id or HIST_Q), n bins between lo and hi."""

    _fields_ = [("value", C.c_int32), ("n", C.c_int32), ("lo", C.c_double), ("hi", C.c_double)]


class HistSpec(C.Structure):
    """Mirror of `ekpnp_hist_spec` (include/ekpnp.h): axis a and an optional axis b (b.n == 0: a 1-D histogram)."""

    _fields_ = [("a", HistAxis), ("b", HistAxis)]

    @property
    def cells(self) -> int:
        return (self.a.n + 2) * (self.b.n + 2 if self.b.n else 1)

    @property
    def cell_shape(self) -> tuple:
        return (self.a.n + 2, self.b.n + 2) if self.b.n else (self.a.n + 2,)


def _hist_axis(axis) -> HistAxis:
    if isinstance(axis, HistAxis):
        return axis
    value, n, lo, hi = axis
    return HistAxis(HIST_VALUE_ID[value] if isinstance(value, str) else int(value), int(n), float(lo), float(hi))


def hist_spec(a, b=None) -> HistSpec:
    """axes as (value name or id, n, lo, hi); value: a field or "q" (c - cn); b None: a 1-D histogram"""
    spec = HistSpec()
    spec.a = _hist_axis(a)
    if b is not None:
        spec.b = _hist_axis(b)
    return spec


def _as_hist_spec(a, b=None) -> HistSpec:
    return a if isinstance(a, HistSpec) else hist_spec(a, b)


def hist_spec_check(p: "Params", spec: HistSpec, planes=None, capacity: int = 1) -> HistSpec:
    """the spec, or EkpnpError with the library's message (ekpnp_hist_spec_check and, when planes = (z_lo, z_hi) is given, the ring's
    ekpnp_hist_range_check: host arithmetic, no device)"""
    L = load_library()
    rc = L.ekpnp_hist_spec_check(C.byref(p), C.byref(spec))
    if rc:
        raise EkpnpError(f"ekpnp_hist_spec_check -> status {rc}: {L.ekpnp_last_error(None).decode()}")
    if planes is not None:
        rc = L.ekpnp_hist_range_check(C.byref(p), int(planes[0]), int(planes[1]), int(capacity))
        if rc:
            raise EkpnpError(f"ekpnp_hist_range_check -> status {rc}: {L.ekpnp_last_error(None).decode()}")
    return spec


def hist_bin(lo: float, hi: float, n: int, v):
    """THE index of v on the axis (lo, hi, n): -1 NaN, 0 below lo, n + 1 at or above hi, else 1 + min(int((v - lo) * (n / (hi - lo))), n - 1)
    (ekpnp_hist_bin, host only; -2 for an axis the spec check refuses).  A scalar gives an int, an array an int32 array."""
    fn = load_library().ekpnp_hist_bin
    if np.ndim(v) == 0:
        return int(fn(float(lo), float(hi), int(n), float(v)))
    a = np.asarray(v, dtype=np.float64)
    return np.fromiter((fn(float(lo), float(hi), int(n), float(x)) for x in a.ravel()), dtype=np.int32, count=a.size).reshape(a.shape)


def hist_edges(axis) -> np.ndarray:
    """the n + 1 edges lo + k (hi - lo) / n of an axis, FOR PLOTTING ONLY: hist_bin is the definition of a bin"""
    ax = _hist_axis(axis)
    return ax.lo + np.arange(ax.n + 1, dtype=np.float64) * (ax.hi - ax.lo) / ax.n


SECTION_Q = 11  # include/ekpnp.h: EKPNP_SECTION_Q, the charge density c - cn as a section value
ACROSS_X, ACROSS_Y = 0, 1  # EKPNP_ACROSS_X (keeps y), EKPNP_ACROSS_Y (keeps x)
MAX_SECTION_PLANES = 16
SECTION_VALUES = FIELDS + ["q"]
SECTION_VALUE_ID = {n: i for i, n in enumerate(SECTION_VALUES)}


class SectionSpec(C.Structure):
    """Mirror of `ekpnp_section_spec` (include/ekpnp.h): a bit mask of values (0: all twelve), the removed axis, its inclusive index
    range, and up to MAX_SECTION_PLANES global z planes (0: every plane of the context, synchronous calls only)."""

    _fields_ = [("values", C.c_uint32), ("across", C.c_int32), ("lo", C.c_int32), ("hi", C.c_int32), ("nplanes", C.c_int32),
                ("z", C.c_int32 * MAX_SECTION_PLANES)]

    @property
    def names(self) -> list:
        return [n for i, n in enumerate(SECTION_VALUES) if self.values == 0 or (self.values >> i) & 1]


def section_spec(values=None, across="x", range=None, planes=None, n=None) -> SectionSpec:
    """values: None (all twelve), a bit mask, or names / ids out of SECTION_VALUES; across: "x" / 0 (keeps y) or "y" / 1 (keeps x);
    range: (lo, hi) inclusive along the removed axis (None: 0 .. n - 1 with n the axis length, which must then be given);
    planes: None (every plane of the context) or global z indices, strictly ascending"""
    spec = SectionSpec()
    if values is None:
        spec.values = 0
    elif isinstance(values, (int, np.integer)):
        spec.values = int(values)
    else:
        mask = 0
        for v in ([values] if isinstance(values, str) else values):
            mask |= 1 << (SECTION_VALUE_ID[v] if isinstance(v, str) else int(v))
        spec.values = mask
    spec.across = {"x": ACROSS_X, "y": ACROSS_Y}[across] if isinstance(across, str) else int(across)
    if range is None:
        if n is None:
            raise ValueError("section_spec: range=None needs the axis length n")
        range = (0, int(n) - 1)
    spec.lo, spec.hi = int(range[0]), int(range[1])
    planes = [] if planes is None else [int(z) for z in planes]
    spec.nplanes = len(planes)
    for j, z in enumerate(planes[:MAX_SECTION_PLANES]):
        spec.z[j] = z
    return spec


def section_spec_check(p: "Params", spec: SectionSpec) -> SectionSpec:
    """the spec, or EkpnpError with the library's message (ekpnp_section_spec_check: host arithmetic, no device)"""
    L = load_library()
    rc = L.ekpnp_section_spec_check(C.byref(p), C.byref(spec))
    if rc:
        raise EkpnpError(f"ekpnp_section_spec_check -> status {rc}: {L.ekpnp_last_error(None).decode()}")
    return spec


def section_extent(p: "Params", spec: SectionSpec):
    """(nvalues, nkeep) of a section (ekpnp_section_extent: host arithmetic, no device)"""
    L = load_library()
    nv, nk = C.c_int(), C.c_int()
    rc = L.ekpnp_section_extent(C.byref(p), C.byref(spec), C.byref(nv), C.byref(nk))
    if rc:
        raise EkpnpError(f"ekpnp_section_extent -> status {rc}: {L.ekpnp_last_error(None).decode()}")
    return nv.value, nk.value


def section_sum(v, stride: int = 1, n: int = None) -> float:
    """THE sum of a line: the terms v[i * stride], i < n, added in runs of 64 consecutive indices, each run in ascending i, the run
    sums in ascending run (ekpnp_section_sum, host only).  n None: as many terms as v holds at that stride."""
    a = np.ascontiguousarray(v, dtype=np.float64).ravel()
    stride = int(stride)
    if n is None:
        n = (a.size + stride - 1) // stride
    if n < 1 or stride < 1 or (int(n) - 1) * stride >= a.size:
        raise ValueError(f"section_sum: n = {n}, stride = {stride} do not fit {a.size} values")
    return float(load_library().ekpnp_section_sum(a.ctypes.data_as(C.c_void_p), stride, int(n)))


def _section_spec_for(p: "Params", values, across, range, planes) -> SectionSpec:
    if isinstance(values, SectionSpec):
        return values
    a = {"x": ACROSS_X, "y": ACROSS_Y}[across] if isinstance(across, str) else int(across)
    return section_spec(values, a, range, planes, n=p.nx if a == ACROSS_X else p.ny)


TRACERS_RANDOM, TRACERS_GRID = 0, 1  # include/ekpnp.h: EKPNP_TRACERS_*
TRACERS_MAX_N = 1 << 28
TRACERS_MAX_CELLS = 65536
TRACER_MOMENTS = ["alive", "lost", "sum_dx", "sum_dy", "sum_dz", "sum_dx2", "sum_dy2", "sum_dz2", "sum_z", "sum_z2", "z_min", "z_max"]
TRACER_MOMENT_ID = {n: i for i, n in enumerate(TRACER_MOMENTS)}


class TracersSpec(C.Structure):
    """Mirror of `ekpnp_tracers_spec` (include/ekpnp.h): n particles, random in a box or on a gx x gy x gz grid of cell centres, the
    noise seed, and the box lo .. hi in lattice units (x, y, z)."""

    _fields_ = [("n", C.c_int64), ("mode", C.c_int32), ("gx", C.c_int32), ("gy", C.c_int32), ("gz", C.c_int32), ("seed", C.c_uint64),
                ("lo", C.c_double * 3), ("hi", C.c_double * 3)]


def tracers_spec(n: int = None, grid=None, box=None, seed: int = 1, p: "Params" = None) -> TracersSpec:
    """n random particles, or grid=(gx, gy, gz) cell centres (n = gx*gy*gz); box: ((x0, x1), (y0, y1), (z0, z1)) in lattice units,
    default the interior [0, nx] x [0, ny] x [1, nz-2] of the lattice p"""
    spec = TracersSpec()
    if grid is not None:
        spec.mode = TRACERS_GRID
        spec.gx, spec.gy, spec.gz = (int(g) for g in grid)
        spec.n = spec.gx * spec.gy * spec.gz if n is None else int(n)
    else:
        if n is None:
            raise ValueError("tracers_spec: n or grid is needed")
        spec.mode = TRACERS_RANDOM
        spec.n = int(n)
    if box is None:
        if p is None:
            raise ValueError("tracers_spec: box=None needs the lattice p")
        box = ((0.0, p.nx), (0.0, p.ny), (1.0, p.nz - 2))
    for a in range(3):
        spec.lo[a], spec.hi[a] = float(box[a][0]), float(box[a][1])
    spec.seed = int(seed)
    return spec


def _tracers_fail(L, name, rc):
    raise EkpnpError(f"{name} -> status {rc}: {L.ekpnp_last_error(None).decode()}")


def tracers_spec_check(p: "Params", spec: TracersSpec) -> TracersSpec:
    """the spec, or EkpnpError with the library's message (ekpnp_tracers_spec_check: host arithmetic, no device)"""
    L = load_library()
    rc = L.ekpnp_tracers_spec_check(C.byref(p), C.byref(spec))
    if rc:
        _tracers_fail(L, "ekpnp_tracers_spec_check", rc)
    return spec


def tracers_seed_host(p: "Params", spec: TracersSpec, first: int = 0, count: int = None):
    """(x, y, z) of particles first .. first + count - 1 of a seed: THE definition (ekpnp_tracers_seed_host, host only)"""
    L = load_library()
    if count is None:
        count = int(spec.n) - int(first)
    x, y, z = (np.zeros(max(int(count), 0), dtype=np.float64) for _ in range(3))
    rc = L.ekpnp_tracers_seed_host(C.byref(p), C.byref(spec), int(first), int(count), _ptr(x), _ptr(y), _ptr(z))
    if rc:
        _tracers_fail(L, "ekpnp_tracers_seed_host", rc)
    return x, y, z


def tracers_advance_host(p: "Params", u, x, y, z, wx=None, wy=None, E=None, mu: float = 0.0, h: float = 0.0, nsub: int = 1):
    """nsub midpoint substeps of h seconds through the frozen arrays u = (ux, uy, uz) [nz, ny, nx] (and E = (Ex, Ey, Ez) when
    mu != 0): THE definition of an advance (ekpnp_tracers_advance_host, host only).  Returns new (x, y, z, wx, wy)."""
    L = load_library()
    shape = (p.nz, p.ny, p.nx)
    u = [np.ascontiguousarray(a, dtype=np.float64).reshape(shape) for a in u]
    e = [None] * 3 if E is None else [np.ascontiguousarray(a, dtype=np.float64).reshape(shape) for a in E]
    x, y, z = (np.array(a, dtype=np.float64).ravel() for a in (x, y, z))
    n = x.size
    wx = np.zeros(n, dtype=np.int32) if wx is None else np.array(wx, dtype=np.int32).ravel()
    wy = np.zeros(n, dtype=np.int32) if wy is None else np.array(wy, dtype=np.int32).ravel()
    if not (y.size == z.size == wx.size == wy.size == n):
        raise ValueError("tracers_advance_host: x, y, z, wx, wy differ in length")
    rc = L.ekpnp_tracers_advance_host(C.byref(p), *[_ptr(a) for a in u], *[None if a is None else _ptr(a) for a in e], float(mu), float(h), int(nsub),
                                      n, _ptr(x), _ptr(y), _ptr(z), _ptr(wx), _ptr(wy))
    if rc:
        _tracers_fail(L, "ekpnp_tracers_advance_host", rc)
    return x, y, z, wx, wy


def stretch_identity(x, y, z):
    """(F [3, 3, n], e [n]) of a record that was just begun: the identity and 0, F = NaN for a lost particle"""
    x, y, z = (np.asarray(a, dtype=np.float64).ravel() for a in (x, y, z))
    F = np.zeros((3, 3, x.size), dtype=np.float64)
    for c in range(3):
        F[c, c] = 1.0
    F[:, :, np.isnan(x) | np.isnan(y) | np.isnan(z)] = np.nan
    return F, np.zeros(x.size, dtype=np.int32)


def tracers_advance_tangent_host(p: "Params", u, x, y, z, F=None, e=None, E=None, mu: float = 0.0, h: float = 0.0, nsub: int = 1, wx=None, wy=None):
    """nsub tangent substeps of h seconds: the positions of tracers_advance_host, bit for bit, and beside them the flow-map gradient
    F [3, 3, n] (row: component of the end point, column: of the start point, lattice coordinates) with its exponent e [n] int32 -
    the true gradient is F * 2^e.  F=None, e=None: a record just begun (stretch_identity).  THE definition of a tangent advance
    (ekpnp_tracers_advance_tangent_host, host only).  Returns new (x, y, z, wx, wy, F, e)."""
    L = load_library()
    shape = (p.nz, p.ny, p.nx)
    u = [np.ascontiguousarray(a, dtype=np.float64).reshape(shape) for a in u]
    ef = [None] * 3 if E is None else [np.ascontiguousarray(a, dtype=np.float64).reshape(shape) for a in E]
    x, y, z = (np.array(a, dtype=np.float64).ravel() for a in (x, y, z))
    n = x.size
    wx = np.zeros(n, dtype=np.int32) if wx is None else np.array(wx, dtype=np.int32).ravel()
    wy = np.zeros(n, dtype=np.int32) if wy is None else np.array(wy, dtype=np.int32).ravel()
    F0, e0 = stretch_identity(x, y, z)
    F = F0 if F is None else np.array(F, dtype=np.float64)
    e = e0 if e is None else np.array(e, dtype=np.int32).ravel()
    if not (y.size == z.size == wx.size == wy.size == e.size == n) or F.size != 9 * n:
        raise ValueError("tracers_advance_tangent_host: x, y, z, wx, wy, F, e differ in length")
    F = np.ascontiguousarray(F.reshape(3, 3, n))
    rc = L.ekpnp_tracers_advance_tangent_host(C.byref(p), *[_ptr(a) for a in u], *[None if a is None else _ptr(a) for a in ef], float(mu), float(h), int(nsub),
                                              n, _ptr(x), _ptr(y), _ptr(z), _ptr(wx), _ptr(wy), _ptr(F), _ptr(e))
    if rc:
        _tracers_fail(L, "ekpnp_tracers_advance_tangent_host", rc)
    return x, y, z, wx, wy, F, e


STRETCH_NO_LEVEL = -2 ** 31  # INT32_MIN: a lost particle, or F = 0


def stretch_level(F, e):
    """floor(log2 of the squared Frobenius norm of F * 2^e) per particle, by integer arithmetic on the bit pattern of the sum of
    squares (ekpnp_stretch_level, host only): the cell rule of tracers_stretch_levels.  STRETCH_NO_LEVEL for NaN or 0.  F is
    [3, 3, n], [9, n], [3, 3] or [9]; an int for one particle, else an int32 array."""
    L = load_library()
    F = np.asarray(F, dtype=np.float64)
    one = F.size == 9
    F = np.array(F.reshape(9, -1).T, dtype=np.float64, order="C")   # [n, 9]: a particle's nine entries side by side
    e = np.asarray(e, dtype=np.int32).ravel()
    if e.size != F.shape[0]:
        raise ValueError("stretch_level: F and e differ in length")
    out = np.empty(e.size, dtype=np.int32)
    base = F.ctypes.data
    for i in range(e.size):
        out[i] = L.ekpnp_stretch_level(base + 72 * i, int(e[i]))
    return int(out[0]) if one else out


def tracers_kick(seed: int, id: int, epoch: int) -> np.ndarray:
    """r[0..2] in (-1, 1): the draw of particle `id` at substep `epoch` of a Brownian advance - one Philox4x32-10 call, exact in
    FP64 (ekpnp_tracers_kick, host only)"""
    r = np.empty(3, dtype=np.float64)
    load_library().ekpnp_tracers_kick(int(seed), int(id), int(epoch), _ptr(r))
    return r


def tracers_advance_brownian_host(p: "Params", u, x, y, z, wx=None, wy=None, E=None, mu: float = 0.0, D: float = 0.0, h: float = 0.0, nsub: int = 1,
                                  seed: int = 0, epoch: int = 0, ids=None):
    """nsub Brownian substeps of h seconds - the midpoint substep of tracers_advance_host, a uniform kick of variance 2 D h, x and y
    folded, z reflected at the plates - with the numbers of (seed, ids[i] or i, epoch .. epoch + nsub - 1): THE definition of a
    Brownian advance (ekpnp_tracers_advance_brownian_host, host only).  Returns new (x, y, z, wx, wy)."""
    L = load_library()
    shape = (p.nz, p.ny, p.nx)
    u = [np.ascontiguousarray(a, dtype=np.float64).reshape(shape) for a in u]
    e = [None] * 3 if E is None else [np.ascontiguousarray(a, dtype=np.float64).reshape(shape) for a in E]
    x, y, z = (np.array(a, dtype=np.float64).ravel() for a in (x, y, z))
    n = x.size
    wx = np.zeros(n, dtype=np.int32) if wx is None else np.array(wx, dtype=np.int32).ravel()
    wy = np.zeros(n, dtype=np.int32) if wy is None else np.array(wy, dtype=np.int32).ravel()
    ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ravel()
    if not (y.size == z.size == wx.size == wy.size == n) or (ids is not None and ids.size != n):
        raise ValueError("tracers_advance_brownian_host: x, y, z, wx, wy, ids differ in length")
    rc = L.ekpnp_tracers_advance_brownian_host(C.byref(p), *[_ptr(a) for a in u], *[None if a is None else _ptr(a) for a in e], n,
                                               None if ids is None else _ptr(ids), _ptr(x), _ptr(y), _ptr(z), _ptr(wx), _ptr(wy),
                                               float(mu), float(D), float(h), int(nsub), int(seed), int(epoch))
    if rc:
        _tracers_fail(L, "ekpnp_tracers_advance_brownian_host", rc)
    return x, y, z, wx, wy


ABSORB_WALLS = {"bottom": 1, "top": 2, "both": 3}


def _absorb_walls(absorb) -> int:
    """the mask of ekpnp_tracers_advance_absorbing: "bottom" (1), "top" (2), "both" (3), or the number itself"""
    if isinstance(absorb, str):
        if absorb not in ABSORB_WALLS:
            raise ValueError(f"absorb = {absorb!r}: expected one of {sorted(ABSORB_WALLS)}")
        return ABSORB_WALLS[absorb]
    return int(absorb)


def landings_empty(n: int):
    """(land_epoch, land_wall, land_x, land_y, land_wx, land_wy) of n particles that never landed"""
    return (np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=np.int32), np.full(n, np.nan), np.full(n, np.nan), np.zeros(n, dtype=np.int32),
            np.zeros(n, dtype=np.int32))


def tracers_advance_absorbing_host(p: "Params", u, x, y, z, wx=None, wy=None, E=None, mu: float = 0.0, D: float = 0.0, h: float = 0.0, nsub: int = 1,
                                   seed: int = 0, epoch: int = 0, ids=None, walls=3, record=None):
    """nsub absorbing substeps of h seconds - Brownian substeps whose plates in `walls` (1: bottom, 2: top, 3: both, or their names)
    keep what reaches them and write its first arrival into the landing record, six arrays indexed by the particle's id (record:
    an earlier record to go on from, never overwritten; None: nobody has landed): THE definition of an absorbing advance
    (ekpnp_tracers_advance_absorbing_host, host only).  Returns new (x, y, z, wx, wy, land_epoch, land_wall, land_x, land_y,
    land_wx, land_wy)."""
    L = load_library()
    shape = (p.nz, p.ny, p.nx)
    u = [np.ascontiguousarray(a, dtype=np.float64).reshape(shape) for a in u]
    e = [None] * 3 if E is None else [np.ascontiguousarray(a, dtype=np.float64).reshape(shape) for a in E]
    x, y, z = (np.array(a, dtype=np.float64).ravel() for a in (x, y, z))
    n = x.size
    wx = np.zeros(n, dtype=np.int32) if wx is None else np.array(wx, dtype=np.int32).ravel()
    wy = np.zeros(n, dtype=np.int32) if wy is None else np.array(wy, dtype=np.int32).ravel()
    ids = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).ravel()
    if record is None:
        rec = landings_empty(n)
    else:
        rec = tuple(np.array(a, dtype=t).ravel() for a, t in zip(record, (np.int64, np.int32, np.float64, np.float64, np.int32, np.int32)))
    if not (y.size == z.size == wx.size == wy.size == n) or (ids is not None and ids.size != n) or len(rec) != 6 or any(a.size != n for a in rec):
        raise ValueError("tracers_advance_absorbing_host: x, y, z, wx, wy, ids and the six record arrays differ in length")
    rc = L.ekpnp_tracers_advance_absorbing_host(C.byref(p), *[_ptr(a) for a in u], *[None if a is None else _ptr(a) for a in e], n,
                                                None if ids is None else _ptr(ids), _ptr(x), _ptr(y), _ptr(z), _ptr(wx), _ptr(wy),
                                                float(mu), float(D), float(h), int(nsub), int(seed), int(epoch), _absorb_walls(walls), *[_ptr(a) for a in rec])
    if rc:
        _tracers_fail(L, "ekpnp_tracers_advance_absorbing_host", rc)
    return (x, y, z, wx, wy, *rec)


def landings_bin(e0: int, width: int, nbins: int, epoch):
    """the cell of an arrival-time histogram: 0 below e0, 1 + (epoch - e0) // width, nbins + 1 from e0 + nbins*width on: THE
    definition (ekpnp_landings_bin, host only, 64-bit integer arithmetic).  An int for a scalar epoch, else an int64 array."""
    L = load_library()
    ep = np.asarray(epoch, dtype=np.int64)
    out = np.empty(ep.size, dtype=np.int64)
    for i, v in enumerate(ep.ravel()):
        out[i] = L.ekpnp_landings_bin(int(e0), int(width), int(nbins), int(v))
    if L.ekpnp_landings_bin(int(e0), int(width), int(nbins), 0) < 0:
        _tracers_fail(L, "ekpnp_landings_bin", 1)
    return int(out[0]) if ep.ndim == 0 else out.reshape(ep.shape)


def tracers_cell(p: "Params", cells, x, y, z) -> np.ndarray:
    """the cell (cz*by + cy)*bx + cx of every position in a cells = (bx, by, bz) partition, -1 for a lost particle: THE definition
    (ekpnp_tracers_cell, host only)"""
    L = load_library()
    bx, by, bz = (int(b) for b in cells)
    x, y, z = (np.asarray(a, dtype=np.float64).ravel() for a in (x, y, z))
    out = np.empty(x.size, dtype=np.int64)
    for i in range(x.size):
        out[i] = L.ekpnp_tracers_cell(C.byref(p), bx, by, bz, float(x[i]), float(y[i]), float(z[i]))
    if x.size and out.min() < -1:
        _tracers_fail(L, "ekpnp_tracers_cell", 1)
    return out


TRACERS_KEY_LOST = 0xFFFFFFFF


def tracers_sort_key(p: "Params", x, y, z) -> np.ndarray:
    """the sort key (k0*ny + j0)*nx + i0 of every position, the linear index of the first node its advance loads; 0xFFFFFFFF for a
    lost particle: THE definition (ekpnp_tracers_sort_key, host only).  uint32, shaped like x."""
    L = load_library()
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    if not (x.shape == y.shape == z.shape):
        raise ValueError("tracers_sort_key: x, y, z differ in shape")
    if L.ekpnp_tracers_sort_host(C.byref(p), 0, None, None, None, None):   # the lattice, checked once
        _tracers_fail(L, "ekpnp_tracers_sort_key", 1)
    out = np.empty(x.size, dtype=np.uint32)
    xs, ys, zs = x.ravel(), y.ravel(), z.ravel()
    for i in range(x.size):
        out[i] = L.ekpnp_tracers_sort_key(C.byref(p), float(xs[i]), float(ys[i]), float(zs[i]))
    return out.reshape(x.shape)


def tracers_sort_host(p: "Params", x, y, z) -> np.ndarray:
    """perm (int32): THE stable ascending order of the sort keys; perm[s] is the slot whose particle moves to slot s, lost particles
    last (ekpnp_tracers_sort_host, host only)"""
    L = load_library()
    x, y, z = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (x, y, z))
    if not (x.size == y.size == z.size):
        raise ValueError("tracers_sort_host: x, y, z differ in length")
    perm = np.empty(x.size, dtype=np.int32)
    rc = L.ekpnp_tracers_sort_host(C.byref(p), x.size, _ptr(x), _ptr(y), _ptr(z), _ptr(perm))
    if rc:
        _tracers_fail(L, "ekpnp_tracers_sort_host", rc)
    return perm


TRACERS_Q = 11  # include/ekpnp.h: EKPNP_TRACERS_Q, the charge density c - cn as a sampled value
TRACERS_MAX_VALUES = 12
TRACERS_MAX_TRACKS = 1024
TRACERS_VALUES = FIELDS + ["q"]
TRACERS_VALUE_ID = {n: i for i, n in enumerate(TRACERS_VALUES)}


class TracksSpec(C.Structure):
    """Mirror of `ekpnp_tracks_spec` (include/ekpnp.h): the tagged particle ids, in the order of the rows, and the values sampled
    at them beside x, y, z, wx, wy."""

    _fields_ = [("ntags", C.c_int32), ("nvalues", C.c_int32), ("values", C.c_int32 * TRACERS_MAX_VALUES), ("ids", C.c_int32 * TRACERS_MAX_TRACKS)]

    def names(self) -> list:
        return [TRACERS_VALUES[self.values[k]] for k in range(self.nvalues)]


def _tracers_values(values) -> np.ndarray:
    """names (of the fields, or "q") or ids, one or several, as the int32 array the library takes; nothing is checked here"""
    if isinstance(values, (str, int, np.integer)):
        values = [values]
    return np.array([TRACERS_VALUE_ID[v] if isinstance(v, str) else int(v) for v in values], dtype=np.int32)


def tracers_values_check(p: "Params", values) -> np.ndarray:
    """the value ids (int32), or EkpnpError with the library's message (ekpnp_tracers_values_check: host arithmetic, no device)"""
    L = load_library()
    ids = _tracers_values(values)
    rc = L.ekpnp_tracers_values_check(C.byref(p), ids.size, _ptr(ids))
    if rc:
        _tracers_fail(L, "ekpnp_tracers_values_check", rc)
    return ids


def tracers_sample_host(p: "Params", values, fields, x, y, z) -> np.ndarray:
    """[nvalues, n]: the values (names or ids) at the positions x, y, z, interpolated in the arrays fields - a dict name -> [nz, ny,
    nx] that holds at least the named ones (q needs c and cn): THE definition of a sample (ekpnp_tracers_sample_host, host only)"""
    L = load_library()
    ids = _tracers_values(values)
    shape = (p.nz, p.ny, p.nx)
    keep = {n: np.ascontiguousarray(a, dtype=np.float64).reshape(shape) for n, a in fields.items()}
    ptrs = (C.c_void_p * len(FIELDS))(*[keep[n].ctypes.data if n in keep else None for n in FIELDS])
    x, y, z = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (x, y, z))
    if not (x.size == y.size == z.size):
        raise ValueError("tracers_sample_host: x, y, z differ in length")
    out = np.empty((ids.size, x.size), dtype=np.float64)
    rc = L.ekpnp_tracers_sample_host(C.byref(p), ids.size, _ptr(ids), ptrs, x.size, _ptr(x), _ptr(y), _ptr(z), _ptr(out))
    if rc:
        _tracers_fail(L, "ekpnp_tracers_sample_host", rc)
    return out


def tracks_spec(ids, values=()) -> TracksSpec:
    """the particles with these ids (ekpnp_tracers_ids' numbering; at most TRACERS_MAX_TRACKS, rows keep this order) and the values
    (names or ids, may be none) sampled at them; nothing is checked here"""
    ids = [int(i) for i in np.asarray(ids).ravel()]
    vals = _tracers_values(values)
    spec = TracksSpec()
    spec.ntags, spec.nvalues = len(ids), int(vals.size)
    for k, v in enumerate(vals[:TRACERS_MAX_VALUES]):
        spec.values[k] = int(v)
    for k, i in enumerate(ids[:TRACERS_MAX_TRACKS]):
        spec.ids[k] = i
    return spec


def tracks_spec_check(p: "Params", n: int, spec: TracksSpec) -> TracksSpec:
    """the spec for a cloud of n particles, or EkpnpError with the library's message (ekpnp_tracks_spec_check: no device)"""
    L = load_library()
    rc = L.ekpnp_tracks_spec_check(C.byref(p), int(n), C.byref(spec))
    if rc:
        _tracers_fail(L, "ekpnp_tracks_spec_check", rc)
    return spec


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class _Diagnostics:
    """The diagnostic methods Solver and Group share (stats.hip, snapshot.hip, monitor.hip, seed.hip, modes.hip, spectrum.hip, hist.hip,
    section.hip): the same calls on a context (ekpnp_*) and on a group (ekpnp_group_*).  The class supplies the prefix (_PREFIX), the
    handle (_handle) and the planes of a per-plane result (_planes: nz_local of a Solver, its own planes; the lattice's nz of a Group,
    where every slab works on its own planes on its own device and the host adds or places the slabs' rows)."""

    def _call(self, name: str, *args):
        self._ck(getattr(self._L, self._PREFIX + name)(self._handle, *args))

    def _count(self, name: str):
        r, d = C.c_int64(), C.c_int64()
        self._call(name, C.byref(r), C.byref(d))
        return int(r.value), int(d.value)

    def _read(self, name: str, first: int, count: int, *rows):
        """labels + typed row arrays: (steps, times, one array [count, *shape] of dtype per (shape, dtype) in rows)"""
        n = max(count, 0)
        steps, times = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.float64)
        out = [np.zeros((n,) + tuple(shape), dtype=dtype) for shape, dtype in rows]
        self._call(name, int(first), int(count), _ptr(steps), _ptr(times), *[_ptr(a) for a in out])
        return (steps, times, *out)

    # -- plane profiles and running statistics (no reference counterpart) --------------------
    def plane_sums(self) -> np.ndarray:
        """[len(PROFILE_NAMES)][planes]: sums over the nx*ny nodes of each plane of the current fields, their squares and the flux /
        body-force products, reduced on the device (a mean is a sum / (nx*ny)).  planes: nz_local of a Solver, its owned planes; NZ of a
        Group, where every slab reduces its own planes on its own device."""
        out = np.empty((len(PROFILE_NAMES), self._planes), dtype=np.float64)
        self._call("plane_sums", _ptr(out))
        return out

    def stats_reset(self):
        self._call("stats_reset")

    def stats_accumulate(self):
        """running sums += plane sums of the current fields; enqueues only (place it between two step() calls)"""
        self._call("stats_accumulate")

    def stats_get(self):
        """(running sums [len(PROFILE_NAMES)][planes], number of samples)"""
        out, n = np.empty((len(PROFILE_NAMES), self._planes), dtype=np.float64), C.c_int()
        self._call("stats_get", _ptr(out), C.byref(n))
        return out, n.value

    def save_profiles(self, path: str, time: float = 0.0):
        """text file of the time-averaged plane means of the planes (ekpnp_save_profiles / ekpnp_group_save_profiles)"""
        self._call("save_profiles", os.fsencode(path), float(time))

    # -- coarsened FP32 snapshots written while the run continues (snapshot() itself differs: Solver, Group) --
    def snapshot_begin(self, path: str, fields=None, coarsen=(1, 1, 1), time: float = 0.0):
        """enqueue a snapshot for the legacy VTK file `path` and return at once (place it between two step() calls);
        snapshot_finish() writes the file.  At most two are pending: a third begin first finishes the oldest."""
        spec = snapshot_spec(fields, coarsen)
        self._call("snapshot_begin", C.byref(spec), os.fsencode(path), float(time))

    def snapshot_finish(self):
        """wait for the copies of the pending snapshots (not for the compute stream) and write their files"""
        self._call("snapshot_finish")

    @property
    def snapshot_pending(self) -> int:
        return int(getattr(self._L, self._PREFIX + "snapshot_pending")(self._handle))

    # -- per-step scalar time series kept on the device (no reference counterpart) --------------
    def monitor_sample(self, quantities=None) -> np.ndarray:
        """the len(MONITOR_NAMES) scalars of the current fields, now (ekpnp_monitor_sample / ekpnp_group_monitor_sample: complete on
        return; columns that are not selected hold 0.0).  Needs no armed monitor and does not touch the ring."""
        out = np.zeros(len(MONITOR_NAMES), dtype=np.float64)
        self._call("monitor_sample", monitor_mask(quantities), _ptr(out))
        return out

    def monitor_arm(self, quantities=None, every: int = 1, capacity: int = 1024):
        """from now on step() appends a row to a ring of `capacity` rows in device memory after every `every`-th step:
        enqueued only, nothing waits.  Arming again resets the ring and the step count."""
        spec = MonitorSpec(monitor_mask(quantities), int(every), int(capacity))
        self._call("monitor_arm", C.byref(spec))

    def monitor_disarm(self):
        self._call("monitor_disarm")

    def monitor_record(self, step: int, time: float):
        """append a row with the caller's labels (hosts that drive stream_collide_save / fast_Poisson themselves); enqueues only"""
        self._call("monitor_record", int(step), float(time))

    def monitor_count(self):
        """(rows recorded since arming, rows lost to overflow); host-known, never synchronises"""
        return self._count("monitor_count")

    def monitor_read(self, first: int = 0, count: int = None):
        """(steps[n], times[n], values[n][len(MONITOR_NAMES)]) of the rows still held, oldest first; count None: all from `first` on"""
        if count is None:
            r, d = self.monitor_count()
            count = r - d - first
        return self._read("monitor_read", first, count, ((len(MONITOR_NAMES),), np.float64))

    def monitor_save(self, path: str):
        self._call("monitor_save", os.fsencode(path))

    # -- seeding x-y structure and tracking chosen x-y modes (no reference counterpart) -----------
    def seed(self, spec: SeedSpec = None, **kw):
        """add a pattern and / or reproducible noise to the selected field arrays on the device (ekpnp_seed / ekpnp_group_seed: enqueues
        only, no field moves; the bits of get_field, seed_host, set_field).  Then fast_Poisson() and init_equilibrium().  spec, or the
        keywords of seed_spec()."""
        spec = spec if spec is not None else seed_spec(**kw)
        self._call("seed", C.byref(spec))

    def mode_amplitudes(self, field="uz", modes=((1, 1),)) -> np.ndarray:
        """[nmodes][planes][2]: per plane (self.nz_local of a Solver, self.p.nz of a Group) a = sum v cos(theta), b = sum v sin(theta),
        theta = 2 pi (m x/nx + n y/ny), unnormalised (ekpnp_mode_amplitudes / ekpnp_group_mode_amplitudes; complete on return).  field may
        be a ModesSpec."""
        spec = _as_modes_spec(field, modes)
        out = np.zeros((max(spec.nmodes, 0), self._planes, 2), dtype=np.float64)
        self._call("mode_amplitudes", C.byref(spec), _ptr(out))
        return out

    def modes_arm(self, field="uz", modes=((1, 1),), capacity: int = 1024):
        """track the energies E = sum_z (a^2 + b^2) of the modes in a ring of `capacity` rows in device memory; rows are appended by
        modes_record() only"""
        spec = _as_modes_spec(field, modes)
        self._call("modes_arm", C.byref(spec), int(capacity))
        self._modes_n = spec.nmodes

    def modes_disarm(self):
        self._call("modes_disarm")

    def modes_record(self, step: int, time: float):
        """append a row with the caller's labels; enqueues only (place it between two step() calls)"""
        self._call("modes_record", int(step), float(time))

    def modes_count(self):
        """(rows recorded since arming, rows lost to overflow); host-known, never synchronises"""
        return self._count("modes_count")

    def modes_read(self, first: int = 0, count: int = None):
        """(steps[n], times[n], energies[n][nmodes]) of the rows still held, oldest first; count None: all from `first` on"""
        if count is None:
            r, d = self.modes_count()
            count = r - d - first
        return self._read("modes_read", first, count, ((getattr(self, "_modes_n", 0),), np.float64))

    def modes_save(self, path: str):
        self._call("modes_save", os.fsencode(path))

    # -- x-y power spectra per plane: shells, peak and their time series (no reference counterpart) --
    def spectrum_shells(self):
        """(shell_of[ny][nx/2 + 1], count[nshell]) of this lattice: the library's own binning (ekpnp_spectrum_shells, host only)"""
        return spectrum_shells(self.p)

    def spectrum_plane(self, field, z: int) -> np.ndarray:
        """P[ny][nx/2 + 1] of the global plane z in rfft2's layout: w (re^2 + im^2), w = 1 for m = 0 and the even Nyquist column, 2
        otherwise, unnormalised (ekpnp_spectrum_plane / ekpnp_group_spectrum_plane; complete on return)"""
        fid = FIELD_ID[field] if isinstance(field, str) else int(field)
        out = np.zeros((self.p.ny, self.p.nx // 2 + 1), dtype=np.float64)
        self._call("spectrum_plane", fid, int(z), _ptr(out))
        return out

    def spectrum(self, field="uz", planes=None):
        """(shells[np][nshell], peaks[np][3]): per plane the shell spectrum E(s) and the dominant mode (m, n signed, P); planes None:
        every plane (self.nz_local of a Solver, self.p.nz of a Group), else the chosen global z (ekpnp_spectrum / ekpnp_group_spectrum;
        complete on return).  field may be a SpectrumSpec."""
        spec = _as_spectrum_spec(field, planes)
        rows = spec.nplanes if spec.nplanes else self._planes
        nshell = self._spectrum_nshell = getattr(self, "_spectrum_nshell", None) or len(self.spectrum_shells()[1])
        shells = np.zeros((max(rows, 0), nshell), dtype=np.float64)
        peaks = np.zeros((max(rows, 0), 3), dtype=np.float64)
        self._call("spectrum", C.byref(spec), _ptr(shells), _ptr(peaks))
        return shells, peaks

    def spectrum_arm(self, field="uz", planes=(0,), capacity: int = 1024):
        """track shells and peak of the chosen planes in a ring of `capacity` rows in device memory; rows are appended by
        spectrum_record() only"""
        spec = _as_spectrum_spec(field, planes)
        self._call("spectrum_arm", C.byref(spec), int(capacity))
        self._spectrum_np = spec.nplanes
        self._spectrum_nshell = len(self.spectrum_shells()[1])

    def spectrum_disarm(self):
        self._call("spectrum_disarm")

    def spectrum_record(self, step: int, time: float):
        """enqueue one row labelled (step, time): nothing waits, the step graph is left alone"""
        self._call("spectrum_record", int(step), float(time))

    def spectrum_count(self):
        """(recorded, dropped); host-known, never synchronises"""
        return self._count("spectrum_count")

    def spectrum_read(self, first: int = 0, count: int = None):
        """(steps[n], times[n], shells[n][nplanes][nshell], peaks[n][nplanes][3]) of the rows still held, oldest first; count None: all
        from `first` on"""
        if count is None:
            r, d = self.spectrum_count()
            count = max(r - d - first, 0)
        nplanes = getattr(self, "_spectrum_np", 0)
        return self._read("spectrum_read", first, count, ((nplanes, getattr(self, "_spectrum_nshell", 0)), np.float64), ((nplanes, 3), np.float64))

    def spectrum_save(self, path: str):
        self._call("spectrum_save", os.fsencode(path))

    # ---- histograms, value ranges and their time series (hist.hip) ----
    def hist_planes(self, a, b=None):
        """(counts[planes, a.n + 2(, b.n + 2)] int64, nonfinite[planes] int64) of every plane (nz_local of a Solver, its owned planes; nz of
        a Group, the lattice's): cell 0 is the underflow, n + 1 the overflow, a node with a NaN in either value goes to nonfinite and to no
        cell (ekpnp_hist_planes / ekpnp_group_hist_planes; complete on return).  a may be a HistSpec."""
        spec = _as_hist_spec(a, b)
        counts = np.zeros((self._planes,) + spec.cell_shape, dtype=np.int64)
        nonfinite = np.zeros(self._planes, dtype=np.int64)
        self._call("hist_planes", C.byref(spec), _ptr(counts), _ptr(nonfinite))
        return counts, nonfinite

    def value_range(self, value):
        """(vmin[planes], vmax[planes]): per plane (as hist_planes) the smallest and largest value that is not NaN (+Inf, -Inf for a plane
        of NaNs); value: a field or "q" (ekpnp_value_range / ekpnp_group_value_range; complete on return)"""
        vid = HIST_VALUE_ID[value] if isinstance(value, str) else int(value)
        vmin, vmax = np.zeros(self._planes, dtype=np.float64), np.zeros(self._planes, dtype=np.float64)
        self._call("value_range", vid, _ptr(vmin), _ptr(vmax))
        return vmin, vmax

    def hist_arm(self, a, b=None, planes=None, capacity: int = 1024):
        """allocate the ring; a row is ONE histogram summed over the global planes planes = (z_lo, z_hi) inclusive (None: the interior
        1 .. nz - 2); from then on rows are appended by hist_record() only"""
        spec = _as_hist_spec(a, b)
        z_lo, z_hi = (1, self.p.nz - 2) if planes is None else (int(planes[0]), int(planes[1]))
        self._call("hist_arm", C.byref(spec), z_lo, z_hi, int(capacity))
        self._hist_spec = spec

    def hist_disarm(self):
        self._call("hist_disarm")

    def hist_record(self, step: int, time: float):
        """append a row labelled (step, time) (enqueues only)"""
        self._call("hist_record", int(step), float(time))

    def hist_count(self):
        """(rows recorded since the arm, rows dropped because the ring was full); never synchronises"""
        return self._count("hist_count")

    def hist_read(self, first: int = 0, count: int = None):
        """(steps, times, counts[count, a.n + 2(, b.n + 2)], nonfinite[count]) of the rows still held, oldest first"""
        if count is None:
            r, d = self.hist_count()
            count = max(r - d - first, 0)
        spec = getattr(self, "_hist_spec", None)
        cells, shape = (spec.cells, spec.cell_shape) if spec is not None else (0, (0,))
        steps, times, rows = self._read("hist_read", first, count, ((cells + 1,), np.int64))
        return steps, times, rows[:, :cells].reshape((len(steps),) + shape).copy(), rows[:, cells].copy()

    def hist_save(self, path: str):
        self._call("hist_save", os.fsencode(path))

    # ---- sections and their time series (section.hip); a group's rows are the owning slab's ----
    def section(self, values=None, across="x", range=None, planes=None):
        """[nvalues, np, nkeep] float64: every selected value (None: all twelve of SECTION_VALUES, in that order) summed along the axis
        `across` ("x" keeps y, "y" keeps x) over the inclusive index range (None: the whole axis; lo == hi: a cut), per plane - np = the
        chosen global planes, or every plane held when planes is None.  Unnormalised; every entry is section_sum of its line
        (ekpnp_section; complete on return).  values may be a SectionSpec."""
        spec = _section_spec_for(self.p, values, across, range, planes)
        rows = spec.nplanes if spec.nplanes else self._planes
        out = np.zeros((len(spec.names), max(rows, 0), self.p.ny if spec.across == ACROSS_X else self.p.nx), dtype=np.float64)
        self._call("section", C.byref(spec), _ptr(out))
        return out

    def section_write(self, path: str, values=None, across="x", range=None, planes=None, time: float = 0.0):
        """the same map as text: a header line, then one row "name z v ..." per value and plane (ekpnp_section_save)"""
        spec = _section_spec_for(self.p, values, across, range, planes)
        self._call("section_save", C.byref(spec), os.fsencode(path), float(time))

    def section_arm(self, values=None, across="x", range=None, planes=(0,), capacity: int = 1024):
        """allocate the ring of rows [nvalues, nplanes, nkeep] for 1 .. 16 chosen planes; rows are appended by section_record() only"""
        spec = _section_spec_for(self.p, values, across, range, planes)
        self._call("section_arm", C.byref(spec), int(capacity))
        self._section_spec = spec

    def section_disarm(self):
        self._call("section_disarm")

    def section_record(self, step: int, time: float):
        """append a row labelled (step, time) (enqueues only)"""
        self._call("section_record", int(step), float(time))

    def section_count(self):
        """(rows recorded since the arm, rows dropped because the ring was full); never synchronises"""
        return self._count("section_count")

    def section_read(self, first: int = 0, count: int = None):
        """(steps, times, values[count, nvalues, nplanes, nkeep]) of the rows still held, oldest first"""
        if count is None:
            r, d = self.section_count()
            count = max(r - d - first, 0)
        spec = getattr(self, "_section_spec", None)
        shape = (0, 0, 0) if spec is None else (len(spec.names), spec.nplanes, self.p.ny if spec.across == ACROSS_X else self.p.nx)
        return self._read("section_read", first, count, (shape, np.float64))

    def section_save(self, path: str):
        """the ring as text: a header line, then one row "step time name z v ..." per held sample, value and plane (ekpnp_section_ring_save)"""
        self._call("section_ring_save", os.fsencode(path))


def _snapshot_names(spec: SnapshotSpec) -> list:
    return [n for i, n in enumerate(FIELDS) if spec.fields == 0 or (spec.fields >> i) & 1]


class Params(C.Structure):
    """Mirror of `ekpnp_params` (include/ekpnp.h)."""

    _fields_ = [(n, C.c_int32) for n in ("nx", "ny", "nz", "n_lattices", "pb_iterations", "in_place")] + [
        (n, C.c_double)
        for n in (
            "Lx Ly Lz dx dy dz CFL dt cs_square rho0 chargeinf voltage voltage2 Ext eps "
            "diffu diffun nu K Kn D Ra TH uw exf kB electron roomT convertCtoCharge "
            "PB_omega V VC VCn VT"
        ).split()
    ]

    def copy(self) -> "Params":
        q = Params()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(Params))
        return q


def library_path() -> str:
    # EKPNP_LIBRARY: A/B a differently built libekpnp.so (tools/sweep.sh); never a fallback
    return os.environ.get("EKPNP_LIBRARY") or os.path.join(_HERE, _LIBNAME)


def exported_symbols() -> list:
    """Names declared `int|size_t|const char* ekpnp_*(` in include/ekpnp.h."""
    hdr = os.path.join(_HERE, "..", "include", "ekpnp.h")
    txt = open(hdr).read()
    return sorted(set(re.findall(r"\b(ekpnp_[a-z0-9_]+)\s*\(", txt)))


_lib = None


def load_library():
    """dlopen libekpnp.so; raises EkpnpError if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise EkpnpError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    try:
        # PyTorch-ROCm is the plumbing for device memory / streams / torch.distributed.  It ships
        # its own HIP runtime + rocFFT; load it first so that one runtime serves the process.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    ctx = C.c_void_p
    i32, dbl, sz = C.c_int, C.c_double, C.c_size_t
    pd = C.POINTER(C.c_double)
    sig = {
        "ekpnp_default_params": (i32, [C.POINTER(Params), i32, i32, i32]),
        "ekpnp_create": (i32, [C.POINTER(Params), C.POINTER(ctx)]),
        "ekpnp_create_slab": (i32, [C.POINTER(Params), i32, i32, C.POINTER(ctx)]),
        "ekpnp_destroy": (i32, [ctx]),
        "ekpnp_last_error": (C.c_char_p, [ctx]),
        "ekpnp_set_stream": (i32, [ctx, C.c_void_p]),
        "ekpnp_synchronize": (i32, [ctx]),
        "ekpnp_bind_field": (i32, [ctx, i32, C.c_void_p]),
        "ekpnp_field_device_ptr": (i32, [ctx, i32, C.POINTER(C.c_void_p)]),
        "ekpnp_set_field": (i32, [ctx, i32, C.c_void_p]),
        "ekpnp_get_field": (i32, [ctx, i32, C.c_void_p]),
        "ekpnp_initialization": (i32, [ctx]),
        "ekpnp_initialization_converged": (i32, [ctx, dbl, i32, C.POINTER(i32), pd]),
        "ekpnp_init_equilibrium": (i32, [ctx]),
        "ekpnp_stream_collide_save": (i32, [ctx, dbl]),
        "ekpnp_fast_poisson": (i32, [ctx]),
        "ekpnp_invalidate_rhs": (i32, [ctx]),
        "ekpnp_step": (i32, [ctx, i32]),
        "ekpnp_get_time": (i32, [ctx, pd]),
        "ekpnp_set_time": (i32, [ctx, dbl]),
        "ekpnp_local_extent": (i32, [ctx, C.POINTER(i32), C.POINTER(i32)]),
        "ekpnp_kernel_timing_enable": (i32, [ctx, i32]),
        "ekpnp_kernel_timing_get": (i32, [ctx, C.POINTER(i32), pd, C.POINTER(C.c_int64)]),
        "ekpnp_phase_timing_get": (i32, [ctx, C.POINTER(i32), pd]),
        "ekpnp_poisson_stage_timing_get": (i32, [ctx, C.POINTER(i32), pd]),
        "ekpnp_plane_transforms": (i32, [ctx, C.POINTER(i32), C.POINTER(i32)]),
        "ekpnp_pass_order": (i32, [ctx, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "ekpnp_device_bytes": (sz, [ctx]),
        "ekpnp_placement_report": (i32, [ctx, C.POINTER(i32), C.POINTER(i32), pd, i32]),
        "ekpnp_graph_state": (i32, [ctx]),
        "ekpnp_debug_sync_enabled": (i32, []),
        "ekpnp_tune": (i32, [ctx, C.c_char_p, i32]),
        "ekpnp_copy_bandwidth": (i32, [ctx, sz, pd]),
        "ekpnp_halo_buffer": (i32, [ctx, i32, C.POINTER(C.c_void_p), C.POINTER(sz)]),
        "ekpnp_halo_pack": (i32, [ctx]),
        "ekpnp_halo_unpack": (i32, [ctx]),
        "ekpnp_phi_halo_buffer": (i32, [ctx, i32, C.POINTER(C.c_void_p), C.POINTER(sz)]),
        "ekpnp_poisson_stage1": (i32, [ctx]),
        "ekpnp_poisson_edge_buffer": (i32, [ctx, i32, C.POINTER(C.c_void_p), C.POINTER(sz)]),
        "ekpnp_poisson_stage2": (i32, [ctx]),
        "ekpnp_phi_halo_pack": (i32, [ctx]),
        "ekpnp_poisson_stage3": (i32, [ctx]),
        "ekpnp_collide_boundary_planes": (i32, [ctx]),
        "ekpnp_collide_interior_planes": (i32, [ctx]),
        "ekpnp_init_fields": (i32, [ctx]),
        "ekpnp_pbe_begin": (i32, [ctx]),
        "ekpnp_pbe_concentrations": (i32, [ctx]),
        "ekpnp_pbe_relax": (i32, [ctx]),
        "ekpnp_pbe_end": (i32, [ctx]),
        "ekpnp_advance_time": (i32, [ctx]),
        "ekpnp_current": (i32, [ctx, pd]),
        "ekpnp_umax": (i32, [ctx, pd]),
        "ekpnp_record_umax": (i32, [ctx, C.c_char_p, i32, dbl]),
        "ekpnp_save_data_tecplot": (i32, [ctx, C.c_char_p, i32, dbl, i32]),
        "ekpnp_save_data_end": (i32, [ctx, C.c_char_p, i32, dbl]),
        "ekpnp_read_data": (i32, [ctx, C.c_char_p, pd]),
        "ekpnp_save_state": (i32, [ctx, C.c_char_p, dbl]),
        "ekpnp_read_state": (i32, [ctx, C.c_char_p, pd]),
        "ekpnp_save_checkpoint": (i32, [ctx, C.c_char_p]),
        "ekpnp_load_checkpoint": (i32, [ctx, C.c_char_p, pd]),
        "ekpnp_group_save_checkpoint": (i32, [ctx, C.c_char_p]),
        "ekpnp_group_load_checkpoint": (i32, [ctx, C.c_char_p, pd]),
        "ekpnp_compute_parameters": (i32, [C.POINTER(Params), pd, pd, pd, pd, pd]),
        "ekpnp_save_scalar": (i32, [ctx, C.c_char_p, i32, C.c_uint, C.c_uint]),
        # the library's own halo transport (RCCL / peer copies)
        "ekpnp_comm_unique_id": (i32, [C.c_void_p]),
        "ekpnp_rccl_available": (i32, []),
        "ekpnp_slab_attach_comm": (i32, [ctx, C.c_void_p]),
        "ekpnp_comm_timing_get": (i32, [ctx, i32, C.POINTER(i32), pd, pd, C.POINTER(sz)]),
        "ekpnp_group_create": (i32, [C.POINTER(Params), i32, C.POINTER(i32), i32, C.POINTER(ctx)]),
        "ekpnp_group_destroy": (i32, [ctx]),
        "ekpnp_group_last_error": (C.c_char_p, [ctx]),
        "ekpnp_group_size": (i32, [ctx]),
        "ekpnp_group_transport": (i32, [ctx]),
        "ekpnp_group_context": (i32, [ctx, i32, C.POINTER(ctx)]),
        "ekpnp_group_device_bytes": (sz, [ctx]),
        "ekpnp_group_synchronize": (i32, [ctx]),
        "ekpnp_group_set_field": (i32, [ctx, i32, C.c_void_p]),
        "ekpnp_group_get_field": (i32, [ctx, i32, C.c_void_p]),
        "ekpnp_group_initialization": (i32, [ctx]),
        "ekpnp_group_initialization_converged": (i32, [ctx, dbl, i32, C.POINTER(i32), pd]),
        "ekpnp_group_init_equilibrium": (i32, [ctx]),
        "ekpnp_group_stream_collide_save": (i32, [ctx, dbl]),
        "ekpnp_group_fast_poisson": (i32, [ctx]),
        "ekpnp_group_step": (i32, [ctx, i32]),
        "ekpnp_group_tune": (i32, [ctx, C.c_char_p, i32]),
        "ekpnp_group_get_time": (i32, [ctx, pd]),
        "ekpnp_group_set_time": (i32, [ctx, dbl]),
        "ekpnp_group_current": (i32, [ctx, pd]),
        "ekpnp_group_umax": (i32, [ctx, pd]),
        "ekpnp_group_record_umax": (i32, [ctx, C.c_char_p, i32, dbl]),
        "ekpnp_group_save_data_tecplot": (i32, [ctx, C.c_char_p, i32, dbl, i32]),
        "ekpnp_group_save_data_end": (i32, [ctx, C.c_char_p, i32, dbl]),
        "ekpnp_group_read_data": (i32, [ctx, C.c_char_p, pd]),
        "ekpnp_group_save_state": (i32, [ctx, C.c_char_p, dbl]),
        "ekpnp_group_read_state": (i32, [ctx, C.c_char_p, pd]),
        # coarsened FP32 snapshots (a context's read also returns its planes)
        "ekpnp_snapshot_extent": (i32, [C.POINTER(Params), C.POINTER(SnapshotSpec), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(sz)]),
        "ekpnp_snapshot_read": (i32, [ctx, C.POINTER(SnapshotSpec), C.c_void_p, C.POINTER(i32), C.POINTER(i32)]),
        "ekpnp_group_snapshot_read": (i32, [ctx, C.POINTER(SnapshotSpec), C.c_void_p]),
        # host arithmetic of the diagnostics
        "ekpnp_monitor_name": (C.c_char_p, [i32]),
        "ekpnp_monitor_spec_check": (i32, [C.POINTER(MonitorSpec)]),
        "ekpnp_seed_spec_check": (i32, [C.POINTER(Params), C.POINTER(SeedSpec)]),
        "ekpnp_seed_uniform": (dbl, [C.c_uint64, C.c_uint64, i32]),
        "ekpnp_seed_host": (i32, [C.POINTER(Params), C.POINTER(SeedSpec), i32, i32, i32, C.c_void_p]),
        "ekpnp_modes_spec_check": (i32, [C.POINTER(Params), C.POINTER(ModesSpec)]),
        "ekpnp_spectrum_spec_check": (i32, [C.POINTER(Params), C.POINTER(SpectrumSpec)]),
        "ekpnp_spectrum_shell_count": (i32, [C.POINTER(Params), C.POINTER(i32)]),
        "ekpnp_spectrum_shells": (i32, [C.POINTER(Params), C.c_void_p, C.c_void_p]),
        "ekpnp_hist_bin": (i32, [dbl, dbl, i32, dbl]),
        "ekpnp_hist_spec_check": (i32, [C.POINTER(Params), C.POINTER(HistSpec)]),
        "ekpnp_hist_range_check": (i32, [C.POINTER(Params), i32, i32, i32]),
        "ekpnp_section_sum": (dbl, [C.c_void_p, C.c_ssize_t, i32]),
        "ekpnp_section_spec_check": (i32, [C.POINTER(Params), C.POINTER(SectionSpec)]),
        "ekpnp_section_extent": (i32, [C.POINTER(Params), C.POINTER(SectionSpec), C.POINTER(i32), C.POINTER(i32)]),
        # Lagrangian tracers: single contexts only (tracers.hip; no group spellings)
        "ekpnp_tracers_spec_check": (i32, [C.POINTER(Params), C.POINTER(TracersSpec)]),
        "ekpnp_tracers_seed_host": (i32, [C.POINTER(Params), C.POINTER(TracersSpec), C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
        "ekpnp_tracers_advance_host": (i32, [C.POINTER(Params)] + [C.c_void_p] * 6 + [dbl, dbl, i32, C.c_int64] + [C.c_void_p] * 5),
        "ekpnp_tracers_cell": (i32, [C.POINTER(Params), i32, i32, i32, dbl, dbl, dbl]),
        "ekpnp_tracers_sort_key": (C.c_uint32, [C.POINTER(Params), dbl, dbl, dbl]),
        "ekpnp_tracers_sort_host": (i32, [C.POINTER(Params), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
        "ekpnp_tracers_sort": (i32, [ctx]),
        "ekpnp_tracers_ids": (i32, [ctx, C.c_void_p]),
        "ekpnp_tracers_seed": (i32, [ctx, C.POINTER(TracersSpec)]),
        "ekpnp_tracers_set": (i32, [ctx, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
        "ekpnp_tracers_get": (i32, [ctx] + [C.c_void_p] * 5),
        "ekpnp_tracers_size": (i32, [ctx, C.POINTER(C.c_int64)]),
        "ekpnp_tracers_release": (i32, [ctx]),
        "ekpnp_tracers_advance": (i32, [ctx, dbl, dbl, i32]),
        "ekpnp_tracers_kick": (None, [C.c_uint64, C.c_int64, C.c_int64, C.c_void_p]),
        "ekpnp_tracers_advance_brownian_host": (i32, [C.POINTER(Params)] + [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 6 + [dbl, dbl, dbl, i32, C.c_uint64, C.c_int64]),
        "ekpnp_tracers_advance_brownian": (i32, [ctx, dbl, dbl, dbl, i32, C.c_uint64]),
        "ekpnp_tracers_epoch": (i32, [ctx, C.POINTER(C.c_int64)]),
        # absorbing plates: the advance, the landing record and its reductions and file
        "ekpnp_tracers_advance_absorbing_host": (i32, [C.POINTER(Params)] + [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 6 + [dbl, dbl, dbl, i32, C.c_uint64, C.c_int64, i32] + [C.c_void_p] * 6),
        "ekpnp_tracers_advance_absorbing": (i32, [ctx, dbl, dbl, dbl, i32, C.c_uint64, i32]),
        "ekpnp_landings_reset": (i32, [ctx]),
        "ekpnp_landings_get": (i32, [ctx] + [C.c_void_p] * 6),
        "ekpnp_landings_bin": (i32, [C.c_int64, C.c_int64, i32, C.c_int64]),
        "ekpnp_landings_hist": (i32, [ctx, i32, C.c_int64, C.c_int64, i32, C.c_void_p, C.POINTER(C.c_int64)]),
        "ekpnp_landings_map": (i32, [ctx, i32, i32, i32, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
        "ekpnp_landings_save": (i32, [ctx, C.c_char_p]),
        "ekpnp_landings_load": (i32, [ctx, C.c_char_p]),
        # the flow-map gradient: the tangent advance, the stretch record, its histogram of levels and its file
        "ekpnp_tracers_advance_tangent_host": (i32, [C.POINTER(Params)] + [C.c_void_p] * 6 + [dbl, dbl, i32, C.c_int64] + [C.c_void_p] * 7),
        "ekpnp_stretch_level": (i32, [C.c_void_p, i32]),
        "ekpnp_tracers_stretch_begin": (i32, [ctx]),
        "ekpnp_tracers_stretch_end": (i32, [ctx]),
        "ekpnp_tracers_advance_tangent": (i32, [ctx, dbl, dbl, i32]),
        "ekpnp_tracers_stretch_get": (i32, [ctx, C.c_void_p, C.c_void_p]),
        "ekpnp_tracers_stretch_levels": (i32, [ctx, i32, i32, C.c_void_p, C.POINTER(C.c_int64)]),
        "ekpnp_tracers_stretch_save": (i32, [ctx, C.c_char_p]),
        "ekpnp_tracers_stretch_load": (i32, [ctx, C.c_char_p]),
        "ekpnp_tracers_save": (i32, [ctx, C.c_char_p, dbl]),
        "ekpnp_tracers_load": (i32, [ctx, C.c_char_p, pd]),
        "ekpnp_tracers_cell_counts": (i32, [ctx, i32, i32, i32, C.c_void_p, C.POINTER(C.c_int64)]),
        "ekpnp_tracers_moments": (i32, [ctx, C.c_void_p]),
        "ekpnp_tracers_arm": (i32, [ctx, i32]),
        "ekpnp_tracers_disarm": (i32, [ctx]),
        "ekpnp_tracers_record": (i32, [ctx, C.c_int64, dbl]),
        "ekpnp_tracers_count": (i32, [ctx, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "ekpnp_tracers_read": (i32, [ctx, C.c_int64, i32, C.c_void_p, C.c_void_p, C.c_void_p]),
        "ekpnp_tracers_ring_save": (i32, [ctx, C.c_char_p]),
        # the fields at the particles, and tracks of tagged particles
        "ekpnp_tracers_values_check": (i32, [C.POINTER(Params), i32, C.c_void_p]),
        "ekpnp_tracers_sample_host": (i32, [C.POINTER(Params), i32, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4),
        "ekpnp_tracers_sample_device": (i32, [ctx, i32, C.c_void_p, C.c_void_p]),
        "ekpnp_tracers_sample": (i32, [ctx, i32, C.c_void_p, C.c_void_p]),
        "ekpnp_tracks_spec_check": (i32, [C.POINTER(Params), C.c_int64, C.POINTER(TracksSpec)]),
        "ekpnp_tracks_arm": (i32, [ctx, C.POINTER(TracksSpec), i32]),
        "ekpnp_tracks_disarm": (i32, [ctx]),
        "ekpnp_tracks_record": (i32, [ctx, C.c_int64, dbl]),
        "ekpnp_tracks_count": (i32, [ctx, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
        "ekpnp_tracks_read": (i32, [ctx, C.c_int64, i32, C.c_void_p, C.c_void_p, C.c_void_p]),
        "ekpnp_tracks_save": (i32, [ctx, C.c_char_p]),
    }
    # the diagnostics a context and a group both have: ekpnp_<name>(ctx, ...) and ekpnp_group_<name>(group, ...) with the same arguments
    series = {  # the verbs of a time series on a ring (csrc/ring.h)
        "disarm": [], "record": [C.c_int64, dbl], "count": [C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
        "read": [C.c_int64, i32, C.c_void_p, C.c_void_p, C.c_void_p],
    }
    both = {
        # plane profiles and running statistics
        "plane_sums": [C.c_void_p], "stats_reset": [], "stats_accumulate": [], "stats_get": [C.c_void_p, C.POINTER(i32)], "save_profiles": [C.c_char_p, dbl],
        "snapshot_begin": [C.POINTER(SnapshotSpec), C.c_char_p, dbl], "snapshot_finish": [], "snapshot_pending": [],
        # per-step scalar time series
        "monitor_sample": [C.c_uint32, C.c_void_p], "monitor_arm": [C.POINTER(MonitorSpec)], "monitor_save": [C.c_char_p],
        # seeding x-y structure; projection onto chosen x-y modes and its time series
        "seed": [C.POINTER(SeedSpec)],
        "mode_amplitudes": [C.POINTER(ModesSpec), C.c_void_p], "modes_arm": [C.POINTER(ModesSpec), i32], "modes_save": [C.c_char_p],
        # x-y power spectra per plane: shells, peak and their time series (a row is read as shells and peaks)
        "spectrum_plane": [i32, i32, C.c_void_p], "spectrum": [C.POINTER(SpectrumSpec), C.c_void_p, C.c_void_p],
        "spectrum_arm": [C.POINTER(SpectrumSpec), i32], "spectrum_save": [C.c_char_p],
        # histograms, value ranges and their time series
        "hist_planes": [C.POINTER(HistSpec), C.c_void_p, C.c_void_p], "value_range": [i32, C.c_void_p, C.c_void_p],
        "hist_arm": [C.POINTER(HistSpec), i32, i32, i32], "hist_save": [C.c_char_p],
        # sections and their time series
        "section": [C.POINTER(SectionSpec), C.c_void_p], "section_save": [C.POINTER(SectionSpec), C.c_char_p, dbl],
        "section_arm": [C.POINTER(SectionSpec), i32], "section_ring_save": [C.c_char_p],
    }
    for kind in ("monitor", "modes", "spectrum", "hist", "section"):
        for verb, args in series.items():
            both[f"{kind}_{verb}"] = args + [C.c_void_p] if (kind, verb) == ("spectrum", "read") else args
    for name, args in both.items():
        sig["ekpnp_" + name] = sig["ekpnp_group_" + name] = (i32, [ctx] + args)
    for name, (res, args) in sig.items():
        fn = getattr(L, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def default_params(nx: int, ny: int, nz: int) -> Params:
    p = Params()
    rc = load_library().ekpnp_default_params(C.byref(p), nx, ny, nz)
    if rc:
        raise EkpnpError(f"ekpnp_default_params({nx},{ny},{nz}) -> {rc}")
    return p


def snapshot_extent(p: Params, fields=None, coarsen=(1, 1, 1)):
    """(X, Y, Z, payload bytes) of a snapshot of the WHOLE lattice (ekpnp_snapshot_extent: host arithmetic, no device);
    raises EkpnpError with the library's message for a spec it refuses"""
    L = load_library()
    spec = snapshot_spec(fields, coarsen)
    X, Y, Z, b = C.c_int(), C.c_int(), C.c_int(), C.c_size_t()
    rc = L.ekpnp_snapshot_extent(C.byref(p), C.byref(spec), C.byref(X), C.byref(Y), C.byref(Z), C.byref(b))
    if rc:
        raise EkpnpError(f"status {rc}: {L.ekpnp_last_error(None).decode()}")
    return X.value, Y.value, Z.value, int(b.value)


def slab_extent(nz: int, rank: int, nranks: int):
    """(first plane, number of planes) owned by `rank`: planes [rank*nz//nranks, (rank+1)*nz//nranks),
    the same rule as ekpnp_create_slab (slabs differ by at most one plane)."""
    if nranks > 1 and nz // nranks < 4:
        raise ValueError("each z slab needs at least 4 planes")
    z0 = rank * nz // nranks
    return z0, (rank + 1) * nz // nranks - z0


def compute_parameters(p: Params) -> dict:
    """compute_parameters (LBM.cu:2419-2446): the dimensionless groups T, M, C, Fe, Pr."""
    v = [C.c_double() for _ in range(5)]
    rc = load_library().ekpnp_compute_parameters(C.byref(p), *[C.byref(x) for x in v])
    if rc:
        raise EkpnpError(f"ekpnp_compute_parameters -> {rc}")
    return dict(zip(("T", "M", "C", "Fe", "Pr"), (x.value for x in v)))


TRANSPORT_AUTO, TRANSPORT_RCCL, TRANSPORT_COPY = 0, 1, 2
UNIQUE_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library: made by ONE rank, handed to all (ekpnp_comm_unique_id)."""
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    rc = load_library().ekpnp_comm_unique_id(buf)
    if rc:
        raise EkpnpError(f"ekpnp_comm_unique_id -> {rc} (librccl.so.1 not loadable?)")
    return buf.raw


def rccl_available() -> str:
    """'' when this process can bind the RCCL library the transport uses (ekpnp_rccl_available: no device, no
    communicator), else the loader's message.  Hosts call it on every rank and agree BEFORE attaching."""
    L = load_library()
    if L.ekpnp_rccl_available() == 0:
        return ""
    return (L.ekpnp_last_error(None) or b"RCCL cannot be bound").decode()


COMM_KINDS = ("halo", "phi", "edge")  # ekpnp_comm_timing_get kinds 0, 1, 2
STAGE_NAMES = ("stage1", "edge_exchange", "stage2", "phi_exchange", "stage3")  # ekpnp_poisson_stage_timing_get


def comm_timing(L, handle, check) -> dict:
    out = {}
    for kind, name in enumerate(COMM_KINDS):
        n, w, t, b = C.c_int(), C.c_double(), C.c_double(), C.c_size_t()
        check(L.ekpnp_comm_timing_get(handle, kind, C.byref(n), C.byref(w), C.byref(t), C.byref(b)))
        out[name] = {"n": n.value, "wait_ms": w.value, "transfer_ms": t.value, "bytes_sent": int(b.value)}
    return out


class Solver(_Diagnostics):
    """One EK-PNP simulation on the current HIP device (or one z slab of it)."""

    _PREFIX = "ekpnp_"  # (_Diagnostics)
    _handle = property(lambda self: self._h)
    _planes = property(lambda self: self.nz_local)

    def __init__(self, params: Params, rank: int = 0, nranks: int = 1, slab: bool = False):
        self._L = load_library()
        self.p = params.copy()
        self._h = C.c_void_p()
        if nranks == 1 and not slab:
            rc = self._L.ekpnp_create(C.byref(self.p), C.byref(self._h))
        else:
            rc = self._L.ekpnp_create_slab(C.byref(self.p), rank, nranks, C.byref(self._h))
        if rc:
            msg = self._L.ekpnp_last_error(None).decode()
            self._h = C.c_void_p()
            raise EkpnpError(f"ekpnp_create failed ({rc}): {msg}")
        z0, nzl = C.c_int(), C.c_int()
        self._ck(self._L.ekpnp_local_extent(self._h, C.byref(z0), C.byref(nzl)))
        self.z0, self.nz_local = z0.value, nzl.value
        self.shape = (self.nz_local, self.p.ny, self.p.nx)
        self.rank, self.nranks = rank, nranks

    # -- plumbing ---------------------------------------------------------------------------
    def _ck(self, rc: int):
        if rc:
            raise EkpnpError(f"status {rc}: {self._L.ekpnp_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            self._L.ekpnp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        return self._h

    @property
    def lib(self):
        return self._L

    def synchronize(self):
        self._ck(self._L.ekpnp_synchronize(self._h))

    def set_stream(self, hip_stream: int):
        self._ck(self._L.ekpnp_set_stream(self._h, C.c_void_p(hip_stream)))

    def graph_state(self) -> int:
        return int(self._L.ekpnp_graph_state(self._h))

    def device_bytes(self) -> int:
        return int(self._L.ekpnp_device_bytes(self._h))

    def placement_report(self) -> dict:
        """{"tried": n, "chosen": i, "sweep_ms": [...]}: the arenas ekpnp_create timed and the one it kept (tried == 0: no search)"""
        n, ch, ms = C.c_int(), C.c_int(), (C.c_double * 8)()
        self._ck(self._L.ekpnp_placement_report(self._h, C.byref(n), C.byref(ch), ms, 8))
        return {"tried": n.value, "chosen": ch.value, "sweep_ms": [round(ms[k], 4) for k in range(n.value)]}

    def copy_bandwidth(self, nbytes: int = 1 << 32) -> float:
        """GB/s (read + write) of a plain contiguous device copy: the measured streaming ceiling."""
        v = C.c_double()
        self._ck(self._L.ekpnp_copy_bandwidth(self._h, int(nbytes), C.byref(v)))
        return v.value

    # -- fields -----------------------------------------------------------------------------
    def get_field(self, name: str) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float64)
        self._ck(self._L.ekpnp_get_field(self._h, FIELD_ID[name], out.ctypes.data_as(C.c_void_p)))
        return out

    def set_field(self, name: str, value):
        a = np.ascontiguousarray(value, dtype=np.float64).reshape(self.shape)
        self._ck(self._L.ekpnp_set_field(self._h, FIELD_ID[name], a.ctypes.data_as(C.c_void_p)))

    def fields(self) -> dict:
        return {n: self.get_field(n) for n in FIELDS}

    def set_fields(self, d: dict):
        for n, v in d.items():
            self.set_field(n, v)

    def field_device_ptr(self, name: str) -> int:
        p = C.c_void_p()
        self._ck(self._L.ekpnp_field_device_ptr(self._h, FIELD_ID[name], C.byref(p)))
        return int(p.value)

    def bind_field(self, name: str, device_ptr: int):
        self._ck(self._L.ekpnp_bind_field(self._h, FIELD_ID[name], C.c_void_p(device_ptr)))

    # -- the reference's host API (LBM.h:159-180) ---------------------------------------------
    def initialization(self):
        self._ck(self._L.ekpnp_initialization(self._h))

    def initialization_converged(self, rel_tol: float = 1e-10, max_sweeps: int = 100000):
        """initialization() with a convergence test; returns (sweeps done, relative residual)."""
        n, r = C.c_int(), C.c_double()
        self._ck(self._L.ekpnp_initialization_converged(self._h, float(rel_tol), int(max_sweeps), C.byref(n), C.byref(r)))
        return n.value, r.value

    def init_equilibrium(self):
        self._ck(self._L.ekpnp_init_equilibrium(self._h))

    def stream_collide_save(self, t: float = 0.0):
        self._ck(self._L.ekpnp_stream_collide_save(self._h, float(t)))

    def fast_Poisson(self):
        self._ck(self._L.ekpnp_fast_poisson(self._h))

    def step(self, n: int = 1):
        self._ck(self._L.ekpnp_step(self._h, int(n)))

    @property
    def t(self) -> float:
        v = C.c_double()
        self._ck(self._L.ekpnp_get_time(self._h, C.byref(v)))
        return v.value

    # -- diagnostics and IO (LBM.cu:2492-2753) -----------------------------------------------
    def current(self) -> float:
        v = C.c_double()
        self._ck(self._L.ekpnp_current(self._h, C.byref(v)))
        return v.value

    def umax(self) -> float:
        v = C.c_double()
        self._ck(self._L.ekpnp_umax(self._h, C.byref(v)))
        return v.value

    def record_umax(self, path: str, time: float, append: bool = True):
        self._ck(self._L.ekpnp_record_umax(self._h, os.fsencode(path), int(append), float(time)))

    def save_data_tecplot(self, path: str, time: float, first: bool = True, append: bool = False):
        self._ck(self._L.ekpnp_save_data_tecplot(self._h, os.fsencode(path), int(append), float(time), int(first)))

    def save_data_end(self, path: str, time: float, append: bool = False):
        self._ck(self._L.ekpnp_save_data_end(self._h, os.fsencode(path), int(append), float(time)))

    def save_scalar(self, name: str, field: str, n: int, nsteps: int = 1000):
        self._ck(self._L.ekpnp_save_scalar(self._h, os.fsencode(name), FIELD_ID[field], int(n), int(nsteps)))

    def read_data(self, path: str) -> float:
        t = C.c_double()
        self._ck(self._L.ekpnp_read_data(self._h, os.fsencode(path), C.byref(t)))
        return t.value

    def save_state(self, path: str, time: float = 0.0):
        """Lossless binary variant of save_data_end (raw FP64 fields of the owned planes)."""
        self._ck(self._L.ekpnp_save_state(self._h, os.fsencode(path), float(time)))

    def read_state(self, path: str) -> float:
        t = C.c_double()
        self._ck(self._L.ekpnp_read_state(self._h, os.fsencode(path), C.byref(t)))
        return t.value

    # -- coarsened FP32 snapshots (no reference counterpart) -----------------------------------
    def snapshot_planes(self, cz: int = 1):
        """(first output plane, number of output planes) of this context for a z sampling step cz: planes k with k*cz owned"""
        k0 = (self.z0 + cz - 1) // cz
        k1 = (self.z0 + self.nz_local - 1) // cz
        return k0, max(0, k1 - k0 + 1)

    def snapshot(self, fields=None, coarsen=(1, 1, 1)) -> dict:
        """name -> float32 [Zlocal][Y][X]: every cz-th plane of this context (both plates kept), means over cx x cy blocks added
        in a fixed order in float64, rounded once to float32 (ekpnp_snapshot_read; complete on return).  The first output
        plane of a slab is snapshot_planes(cz)[0]."""
        spec = snapshot_spec(fields, coarsen)
        if self._L.ekpnp_snapshot_extent(C.byref(self.p), C.byref(spec), None, None, None, None):
            raise EkpnpError(f"status 1: {self._L.ekpnp_last_error(None).decode()}")
        names = _snapshot_names(spec)
        X, Y = self.p.nx // spec.cx, self.p.ny // spec.cy
        out = np.empty((len(names), self.snapshot_planes(spec.cz)[1], Y, X), dtype=np.float32)
        k0, kn = C.c_int(), C.c_int()
        self._ck(self._L.ekpnp_snapshot_read(self._h, C.byref(spec), out.ctypes.data_as(C.c_void_p), C.byref(k0), C.byref(kn)))
        assert (k0.value, kn.value) == self.snapshot_planes(spec.cz)
        return {n: out[i] for i, n in enumerate(names)}

    # -- Lagrangian tracers: one particle cloud per single context (tracers.hip; slab contexts and groups are refused) --
    def tracers_seed(self, spec: TracersSpec = None, **kw):
        """make the cloud on the device: tracers_seed(spec) or tracers_seed(n=..., grid=..., box=..., seed=...); enqueues only"""
        if spec is None:
            spec = tracers_spec(p=self.p, **kw)
        self._call("tracers_seed", C.byref(spec))

    def tracers_set(self, x, y, z):
        """replace the cloud by these positions (lattice units; all-NaN: a lost particle); start positions = positions, image counts 0"""
        x, y, z = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (x, y, z))
        if not (x.size == y.size == z.size):
            raise ValueError("tracers_set: x, y, z differ in length")
        self._call("tracers_set", x.size, _ptr(x), _ptr(y), _ptr(z))

    @property
    def tracers_size(self) -> int:
        n = C.c_int64()
        self._call("tracers_size", C.byref(n))
        return int(n.value)

    def tracers_get(self, by_id: bool = False):
        """(x, y, z, wx, wy): positions in lattice units (NaN: lost) and the counts of periodic images crossed; synchronises.
        by_id=True: in the original particle order, whatever tracers_sort() did to the slots (un-permuted on the host)"""
        n = self.tracers_size
        x, y, z = (np.empty(n, dtype=np.float64) for _ in range(3))
        wx, wy = (np.empty(n, dtype=np.int32) for _ in range(2))
        self._call("tracers_get", _ptr(x), _ptr(y), _ptr(z), _ptr(wx), _ptr(wy))
        if not by_id:
            return x, y, z, wx, wy
        ids = self.tracers_ids()
        out = []
        for a in (x, y, z, wx, wy):
            o = np.empty_like(a)
            o[ids] = a
            out.append(o)
        return tuple(out)

    def tracers_sort(self):
        """put the cloud into memory order: all its arrays permuted by tracers_sort_host of the current positions; enqueues only.
        No trajectory changes; tracers_ids() / tracers_get(by_id=True) give the particles their original indices back."""
        self._call("tracers_sort")

    def tracers_ids(self) -> np.ndarray:
        """ids[s]: the index the particle in slot s had when the cloud was last seeded, set or loaded (int32); synchronises"""
        ids = np.empty(self.tracers_size, dtype=np.int32)
        self._call("tracers_ids", _ptr(ids))
        return ids

    def tracers_release(self):
        self._call("tracers_release")

    def tracers_advance(self, h: float, nsub: int = 1, mu: float = 0.0, D: float = None, seed: int = 0, absorb=None, stretch: bool = False):
        """nsub midpoint substeps of h seconds through the current, frozen fields with velocity u + mu E; enqueues only (place it
        between two step() calls).  mu != 0 brings a lazy solve's E arrays up to date first.  With a diffusivity D (m^2/s, 0.0
        allowed) every substep also kicks the particle by the numbers of (seed, its id, the cloud's epoch) and reflects it at the
        plates (ekpnp_tracers_advance_brownian); D=None is the deterministic advance.  absorb="bottom", "top" or "both": those
        plates keep what reaches them and the first arrival of every particle goes into the landing record (landings_*;
        ekpnp_tracers_advance_absorbing; D=None then means 0.0: drift alone deposits).  stretch=True: the deterministic advance,
        which also carries the flow-map gradient of the stretch record along (tracers_stretch_begin first;
        ekpnp_tracers_advance_tangent); not together with D= or absorb=."""
        if stretch:
            if D is not None or absorb is not None:
                raise ValueError("tracers_advance: stretch=True goes with the deterministic advance only, not with D= or absorb=")
            self._call("tracers_advance_tangent", float(mu), float(h), int(nsub))
        elif absorb is not None:
            self._call("tracers_advance_absorbing", float(mu), 0.0 if D is None else float(D), float(h), int(nsub), int(seed), _absorb_walls(absorb))
        elif D is None:
            self._call("tracers_advance", float(mu), float(h), int(nsub))
        else:
            self._call("tracers_advance_brownian", float(mu), float(D), float(h), int(nsub), int(seed))

    def tracers_stretch_begin(self):
        """make the stretch record of the cloud, or reset it: F = the identity, e = 0 (F = NaN for a lost particle); enqueues only"""
        self._call("tracers_stretch_begin")

    def tracers_stretch_end(self):
        """drop the stretch record"""
        self._call("tracers_stretch_end")

    def tracers_stretch_get(self, by_id: bool = False):
        """(F [3, 3, n], e [n] int32): the flow-map gradient F * 2^e of every particle over the tangent advances since
        tracers_stretch_begin, in lattice coordinates (NaN: lost); synchronises.  The record is kept in slot order, the order of
        tracers_get(); by_id=True: in the original particle order."""
        n = self.tracers_size
        F, e = np.empty((3, 3, n), dtype=np.float64), np.empty(n, dtype=np.int32)
        self._call("tracers_stretch_get", _ptr(F), _ptr(e))
        if not by_id:
            return F, e
        ids = self.tracers_ids()
        Fo, eo = np.empty_like(F), np.empty_like(e)
        Fo[:, :, ids] = F
        eo[ids] = e
        return Fo, eo

    def tracers_stretch_levels(self, l_lo: int, nlevels: int):
        """(counts [nlevels + 2] int64, none): the particles per level (stretch_level) below l_lo, at l_lo .. l_lo + nlevels - 1, and
        at or above l_lo + nlevels, and those without a level (lost, or F = 0); exact, counts.sum() + none == n"""
        counts, none = np.zeros(max(int(nlevels), 0) + 2, dtype=np.int64), C.c_int64()
        self._call("tracers_stretch_levels", int(l_lo), int(nlevels), _ptr(counts), C.byref(none))
        return counts, int(none.value)

    def tracers_stretch_save(self, path: str):
        self._call("tracers_stretch_save", os.fsencode(path))

    def tracers_stretch_load(self, path: str):
        """needs a cloud of the file's n (after tracers_load, which drops the record); replaces or creates the record"""
        self._call("tracers_stretch_load", os.fsencode(path))

    def tracers_ftle(self, T: float, by_id: bool = False):
        """(ftle [n], det [n]): the finite-time Lyapunov exponent (ln sigma + e ln 2) / |T| of every particle, sigma the largest
        singular value of D F D^-1 with D = diag(dx, dy, dz) (the gradient in physical coordinates), and det F * 2^(3e), which a
        solenoidal flow keeps near 1 (the trilinear interpolant of a solenoidal field is not solenoidal: it drifts).  NaN for a
        lost particle.  Computed in numpy on the fetched record; synchronises."""
        F, e = self.tracers_stretch_get(by_id=by_id)
        d = np.array([self.p.dx, self.p.dy, self.p.dz], dtype=np.float64)
        A = np.moveaxis(F, 2, 0) * (d[:, None] / d[None, :])     # [n, 3, 3]
        ok = np.isfinite(A).all(axis=(1, 2))
        sigma = np.full(e.size, np.nan)
        det = np.full(e.size, np.nan)
        if ok.any():
            sigma[ok] = np.linalg.svd(A[ok], compute_uv=False)[:, 0]
            det[ok] = np.ldexp(np.linalg.det(A[ok]), 3 * e[ok].astype(np.int64))
        with np.errstate(divide="ignore"):
            ftle = (np.log(sigma) + e * np.log(2.0)) / abs(float(T))
        return ftle, det

    def landings_get(self, by_id: bool = True):
        """(land_epoch, land_wall, land_x, land_y, land_wx, land_wy): the first arrival of every particle at an absorbing plate (-1,
        0, NaN, NaN, 0, 0: none yet); synchronises.  The record is kept by particle id; by_id=False gives it in slot order, the
        order of tracers_get()."""
        n = self.tracers_size
        rec = (np.empty(n, dtype=np.int64), np.empty(n, dtype=np.int32), np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64),
               np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32))
        self._call("landings_get", *[_ptr(a) for a in rec])
        if by_id:
            return rec
        ids = self.tracers_ids()
        return tuple(a[ids] for a in rec)

    def landings_hist(self, e0: int = 0, width: int = 1, nbins: int = 1, absorb="both"):
        """(counts [nbins + 2] int64, none): the landings on the plates of `absorb` per cell of landings_bin(e0, width, nbins, epoch),
        and everybody else; exact, counts.sum() + none == n"""
        counts, none = np.zeros(max(int(nbins), 0) + 2, dtype=np.int64), C.c_int64()
        self._call("landings_hist", _absorb_walls(absorb), int(e0), int(width), int(nbins), _ptr(counts), C.byref(none))
        return counts, int(none.value)

    def landings_map(self, wall, cells, e_lo: int = 0, e_hi: int = 2 ** 63 - 1):
        """(counts [by, bx] int64, elsewhere): the landings on one plate ("bottom" / 1 or "top" / 2) with e_lo <= epoch <= e_hi per
        cell of a cells = (bx, by) partition of the plate, by tracers_cell's rule; exact, counts.sum() + elsewhere == n"""
        bx, by = (int(b) for b in cells)
        counts, other = np.zeros((max(by, 0), max(bx, 0)), dtype=np.int64), C.c_int64()
        self._call("landings_map", _absorb_walls(wall), bx, by, int(e_lo), int(e_hi), _ptr(counts), C.byref(other))
        return counts, int(other.value)

    def landings_save(self, path: str):
        self._call("landings_save", os.fsencode(path))

    def landings_load(self, path: str):
        """after tracers_load of the cloud it belongs to (which drops the record)"""
        self._call("landings_load", os.fsencode(path))

    def landings_reset(self):
        """nobody has landed; enqueues only"""
        self._call("landings_reset")

    def tracers_epoch(self) -> int:
        """Brownian substeps taken since the cloud was seeded or set (a load restores the file's): the clock of the noise"""
        e = C.c_int64()
        self._call("tracers_epoch", C.byref(e))
        return int(e.value)

    def tracers_save(self, path: str, time: float = 0.0):
        self._call("tracers_save", os.fsencode(path), float(time))

    def tracers_load(self, path: str) -> float:
        t = C.c_double()
        self._call("tracers_load", os.fsencode(path), C.byref(t))
        return t.value

    def tracers_cell_counts(self, cells):
        """(counts [bz, by, bx] int64, lost): the alive particles per cell of a cells = (bx, by, bz) partition; exact"""
        bx, by, bz = (int(b) for b in cells)
        counts, lost = np.zeros((max(bz, 0), max(by, 0), max(bx, 0)), dtype=np.int64), C.c_int64()
        self._call("tracers_cell_counts", bx, by, bz, _ptr(counts), C.byref(lost))
        return counts, int(lost.value)

    def tracers_moments(self) -> np.ndarray:
        """the len(TRACER_MOMENTS) moments of the cloud, now (unwrapped displacements in lattice units); complete on return"""
        out = np.zeros(len(TRACER_MOMENTS), dtype=np.float64)
        self._call("tracers_moments", _ptr(out))
        return out

    def tracers_arm(self, capacity: int = 1024):
        """allocate the ring of rows of len(TRACER_MOMENTS) moments; rows are appended by tracers_record() only"""
        self._call("tracers_arm", int(capacity))

    def tracers_disarm(self):
        self._call("tracers_disarm")

    def tracers_record(self, step: int, time: float):
        """append the cloud's moments with the caller's labels; enqueues only"""
        self._call("tracers_record", int(step), float(time))

    def tracers_count(self):
        """(rows recorded since arming, rows lost to overflow)"""
        return self._count("tracers_count")

    def tracers_read(self, first: int = 0, count: int = None):
        """(steps, times, values [count, len(TRACER_MOMENTS)]) of the held rows first .. first + count - 1, oldest first"""
        if count is None:
            r, d = self.tracers_count()
            count = r - d - first
        return self._read("tracers_read", first, count, ((len(TRACER_MOMENTS),), np.float64))

    def tracers_ring_save(self, path: str):
        """the ring as text: two header lines, then one row "step time moments ..." per held sample (ekpnp_tracers_ring_save)"""
        self._call("tracers_ring_save", os.fsencode(path))

    def tracers_sample(self, values, by_id: bool = False) -> np.ndarray:
        """[nvalues, n]: the values (names of the fields or "q", or ids) at the particles, interpolated as an advance does; complete on
        return.  Slot order; by_id=True: in the original particle order (un-permuted on the host, like tracers_get)"""
        ids = _tracers_values(values)
        out = np.empty((ids.size, self.tracers_size), dtype=np.float64)
        self._call("tracers_sample", ids.size, _ptr(ids), _ptr(out))
        if not by_id:
            return out
        back = np.empty_like(out)
        back[:, self.tracers_ids()] = out
        return back

    def tracers_sample_into(self, values, out):
        """enqueue the same pass into device memory [nvalues, n] float64, slot order: a contiguous torch tensor on this device, or a raw
        device pointer (int); nothing is allocated and nothing waits"""
        ids = _tracers_values(values)
        if hasattr(out, "data_ptr"):
            if str(out.dtype) != "torch.float64" or not out.is_contiguous() or out.numel() < ids.size * self.tracers_size:
                raise ValueError("tracers_sample_into: a contiguous float64 tensor of at least nvalues * n elements is needed")
            out = out.data_ptr()
        self._call("tracers_sample_device", ids.size, _ptr(ids), C.c_void_p(int(out)))

    def tracks_arm(self, spec: TracksSpec = None, capacity: int = 1024, **kw):
        """allocate the ring of rows [ntags, 5 + nvalues]: tracks_arm(spec) or tracks_arm(ids=..., values=...); rows are appended by
        tracks_record() only"""
        if spec is None:
            spec = tracks_spec(**kw)
        self._call("tracks_arm", C.byref(spec), int(capacity))
        self._tracks_shape = (int(spec.ntags), 5 + int(spec.nvalues))

    def tracks_disarm(self):
        self._call("tracks_disarm")

    def tracks_record(self, step: int, time: float):
        """append x, y, z, wx, wy and the armed values of every tagged particle with the caller's labels; enqueues only"""
        self._call("tracks_record", int(step), float(time))

    def tracks_count(self):
        """(rows recorded since arming, rows lost to overflow)"""
        return self._count("tracks_count")

    def tracks_read(self, first: int = 0, count: int = None):
        """(steps, times, values [count, ntags, 5 + nvalues]) of the held rows first .. first + count - 1, oldest first"""
        if count is None:
            r, d = self.tracks_count()
            count = r - d - first
        return self._read("tracks_read", first, count, (getattr(self, "_tracks_shape", (0, 5)), np.float64))

    def tracks_save(self, path: str):
        """the ring as text: two header lines, then one line "step time id x y z wx wy values ..." per held row and tag (ekpnp_tracks_save)"""
        self._call("tracks_save", os.fsencode(path))

    def tune(self, knob: str, value: int):
        self._ck(self._L.ekpnp_tune(self._h, knob.encode(), int(value)))

    def invalidate_rhs(self):
        self._ck(self._L.ekpnp_invalidate_rhs(self._h))

    def attach_comm(self, unique_id: bytes):
        """Collective over the ranks (ncclCommInitRank): from here on the reference's verbs
        (initialization, stream_collide_save, fast_Poisson, step, current, umax, the writers)
        work on this slab context, the library moving the halos over RCCL itself."""
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError("unique id must be 128 bytes")
        self._ck(self._L.ekpnp_slab_attach_comm(self._h, C.c_char_p(unique_id)))

    def save_checkpoint(self, path: str):
        """fields + post-collision populations: load_checkpoint continues the run bit for bit"""
        self._ck(self._L.ekpnp_save_checkpoint(self._h, os.fsencode(path)))

    def load_checkpoint(self, path: str) -> float:
        t = C.c_double()
        self._ck(self._L.ekpnp_load_checkpoint(self._h, os.fsencode(path), C.byref(t)))
        return t.value

    # -- z-slab pieces: the split entry points (a host's own transport, examples/host_transport.py; tests) ------
    def call(self, name: str):
        """Invoke a parameterless `int ekpnp_<name>(ctx)` entry point."""
        self._ck(getattr(self._L, "ekpnp_" + name)(self._h))

    def buffer(self, kind: str, which: int):
        """(device pointer, n_doubles) of a halo / phi-halo / edge buffer."""
        p, n = C.c_void_p(), C.c_size_t()
        fn = {"halo": self._L.ekpnp_halo_buffer, "phi": self._L.ekpnp_phi_halo_buffer, "edge": self._L.ekpnp_poisson_edge_buffer}[kind]
        self._ck(fn(self._h, which, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    # -- measurement ------------------------------------------------------------------------
    def kernel_timing(self, enable: bool):
        self._ck(self._L.ekpnp_kernel_timing_enable(self._h, int(enable)))

    def phase_timing_get(self):
        """(number of Poisson solves bracketed since the last call, their summed duration in ms)"""
        n, ms = C.c_int(), C.c_double()
        self._ck(self._L.ekpnp_phase_timing_get(self._h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def plane_transforms(self) -> dict:
        """{"own_passes": the library's own row / column kernels (else rocFFT plans), "ranks_on_device": ranks of the lattice
        sharing this context's device (known once a communicator is attached)}"""
        own, n = C.c_int(), C.c_int()
        self._ck(self._L.ekpnp_plane_transforms(self._h, C.byref(own), C.byref(n)))
        return {"own_passes": bool(own.value), "ranks_on_device": n.value}

    def pass_order(self) -> dict:
        """the cache-aware orders in effect: {"band_rows": rows per band of the interior sweep (0: plane after plane),
        "poisson_blocks": kx column blocks of the solve's middle passes, "poisson_zchunk": always 0 (plane chunks are retired)}"""
        b, nb, zc = C.c_int(), C.c_int(), C.c_int()
        self._ck(self._L.ekpnp_pass_order(self._h, C.byref(b), C.byref(nb), C.byref(zc)))
        return {"band_rows": b.value, "poisson_blocks": nb.value, "poisson_zchunk": zc.value}

    def poisson_stage_timing_get(self):
        """Slab contexts: (n solves, {"stage1", "edge_exchange", "stage2", "phi_exchange", "stage3"}: summed ms) of the
        solves bracketed so far - call BEFORE phase_timing_get, which resets them."""
        n, ms = C.c_int(), (C.c_double * 5)()
        self._ck(self._L.ekpnp_poisson_stage_timing_get(self._h, C.byref(n), ms))
        return n.value, dict(zip(STAGE_NAMES, (float(v) for v in ms)))

    def kernel_timing_get(self):
        n, ms, nodes = C.c_int(), C.c_double(), C.c_int64()
        self._ck(self._L.ekpnp_kernel_timing_get(self._h, C.byref(n), C.byref(ms), C.byref(nodes)))
        return n.value, ms.value, nodes.value

    def comm_timing_get(self) -> dict:
        """Per exchange kind of a slab with a transport, since kernel_timing(True): {"halo"|"phi"|"edge":
        {"n", "wait_ms", "transfer_ms", "bytes_sent"}} - sums over the n exchanges, bytes per exchange."""
        return comm_timing(self._L, self._h, self._ck)


class Group(_Diagnostics):
    """nslabs z slabs driven by ONE process (ekpnp_group_*): slab i on HIP device devices[i]
    (default: i modulo the device count; devices may repeat, then the halos move by device copies).
    Same method names as Solver; fields are whole-lattice arrays [NZ][NY][NX]."""

    _PREFIX = "ekpnp_group_"  # (_Diagnostics)
    _handle = property(lambda self: self._g)
    _planes = property(lambda self: self.p.nz)

    def __init__(self, params: Params, nslabs: int, devices=None, transport: int = TRANSPORT_AUTO):
        self._L = load_library()
        self.p = params.copy()
        self._g = C.c_void_p()
        dev = None
        if devices is not None:
            if len(devices) != nslabs:
                raise ValueError("one device per slab")
            dev = (C.c_int * nslabs)(*devices)
        rc = self._L.ekpnp_group_create(C.byref(self.p), int(nslabs), dev, int(transport), C.byref(self._g))
        if rc:
            msg = self._L.ekpnp_group_last_error(None).decode()
            self._g = C.c_void_p()
            raise EkpnpError(f"ekpnp_group_create failed ({rc}): {msg}")
        self.n = nslabs
        self.shape = (self.p.nz, self.p.ny, self.p.nx)
        self.transport = int(self._L.ekpnp_group_transport(self._g))

    def _ck(self, rc: int):
        if rc:
            raise EkpnpError(f"status {rc}: {self._L.ekpnp_group_last_error(self._g).decode()}")

    def close(self):
        if getattr(self, "_g", None):
            self._L.ekpnp_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def slab_handle(self, i: int):
        h = C.c_void_p()
        self._ck(self._L.ekpnp_group_context(self._g, int(i), C.byref(h)))
        return h

    def slab_extent(self, i: int):
        z0, nzl = C.c_int(), C.c_int()
        rc = self._L.ekpnp_local_extent(self.slab_handle(i), C.byref(z0), C.byref(nzl))
        if rc:
            raise EkpnpError(f"ekpnp_local_extent -> {rc}")
        return z0.value, nzl.value

    def device_bytes(self) -> int:
        return int(self._L.ekpnp_group_device_bytes(self._g))

    # measurement: the hooks are per slab context
    def kernel_timing(self, enable: bool):
        for i in range(self.n):
            self._slab_ck(i, self._L.ekpnp_kernel_timing_enable(self.slab_handle(i), int(enable)))

    def slab_kernel_timing_get(self, i: int):
        n, ms, nodes = C.c_int(), C.c_double(), C.c_int64()
        self._slab_ck(i, self._L.ekpnp_kernel_timing_get(self.slab_handle(i), C.byref(n), C.byref(ms), C.byref(nodes)))
        return n.value, ms.value, nodes.value

    def slab_phase_timing_get(self, i: int):
        n, ms = C.c_int(), C.c_double()
        self._slab_ck(i, self._L.ekpnp_phase_timing_get(self.slab_handle(i), C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def slab_comm_timing_get(self, i: int) -> dict:
        h = self.slab_handle(i)
        return comm_timing(self._L, h, lambda rc: self._slab_ck(i, rc))

    def _slab_ck(self, i: int, rc: int):
        if rc:
            raise EkpnpError(f"slab {i}: status {rc}: {self._L.ekpnp_last_error(self.slab_handle(i)).decode()}")

    def synchronize(self):
        self._ck(self._L.ekpnp_group_synchronize(self._g))

    def get_field(self, name: str) -> np.ndarray:
        out = np.empty(self.shape, dtype=np.float64)
        self._ck(self._L.ekpnp_group_get_field(self._g, FIELD_ID[name], out.ctypes.data_as(C.c_void_p)))
        return out

    def set_field(self, name: str, value):
        a = np.ascontiguousarray(value, dtype=np.float64).reshape(self.shape)
        self._ck(self._L.ekpnp_group_set_field(self._g, FIELD_ID[name], a.ctypes.data_as(C.c_void_p)))

    def fields(self) -> dict:
        return {n: self.get_field(n) for n in FIELDS}

    def set_fields(self, d: dict):
        for n, v in d.items():
            self.set_field(n, v)

    def initialization(self):
        self._ck(self._L.ekpnp_group_initialization(self._g))

    def initialization_converged(self, rel_tol: float = 1e-10, max_sweeps: int = 100000):
        n, r = C.c_int(), C.c_double()
        self._ck(self._L.ekpnp_group_initialization_converged(self._g, float(rel_tol), int(max_sweeps), C.byref(n), C.byref(r)))
        return n.value, r.value

    def init_equilibrium(self):
        self._ck(self._L.ekpnp_group_init_equilibrium(self._g))

    def stream_collide_save(self, t: float = 0.0):
        self._ck(self._L.ekpnp_group_stream_collide_save(self._g, float(t)))

    def fast_Poisson(self):
        self._ck(self._L.ekpnp_group_fast_poisson(self._g))

    def tune(self, knob: str, value: int):
        """ekpnp_tune's slab and transport knobs on every slab of the group"""
        self._ck(self._L.ekpnp_group_tune(self._g, knob.encode(), int(value)))

    def step(self, n: int = 1):
        self._ck(self._L.ekpnp_group_step(self._g, int(n)))

    @property
    def t(self) -> float:
        v = C.c_double()
        self._ck(self._L.ekpnp_group_get_time(self._g, C.byref(v)))
        return v.value

    def current(self) -> float:
        v = C.c_double()
        self._ck(self._L.ekpnp_group_current(self._g, C.byref(v)))
        return v.value

    def umax(self) -> float:
        v = C.c_double()
        self._ck(self._L.ekpnp_group_umax(self._g, C.byref(v)))
        return v.value

    def record_umax(self, path: str, time: float, append: bool = True):
        self._ck(self._L.ekpnp_group_record_umax(self._g, os.fsencode(path), int(append), float(time)))

    def save_data_tecplot(self, path: str, time: float, first: bool = True, append: bool = False):
        self._ck(self._L.ekpnp_group_save_data_tecplot(self._g, os.fsencode(path), int(append), float(time), int(first)))

    def save_data_end(self, path: str, time: float, append: bool = False):
        self._ck(self._L.ekpnp_group_save_data_end(self._g, os.fsencode(path), int(append), float(time)))

    def read_data(self, path: str) -> float:
        t = C.c_double()
        self._ck(self._L.ekpnp_group_read_data(self._g, os.fsencode(path), C.byref(t)))
        return t.value

    def save_state(self, path: str, time: float = 0.0):
        self._ck(self._L.ekpnp_group_save_state(self._g, os.fsencode(path), float(time)))

    def read_state(self, path: str) -> float:
        t = C.c_double()
        self._ck(self._L.ekpnp_group_read_state(self._g, os.fsencode(path), C.byref(t)))
        return t.value

    def snapshot(self, fields=None, coarsen=(1, 1, 1)) -> dict:
        """name -> float32 [Z][Y][X] of the whole lattice: every slab coarsens and lands its own sampled planes"""
        spec = snapshot_spec(fields, coarsen)
        X, Y, Z, _ = snapshot_extent(self.p, spec.fields, coarsen)
        names = _snapshot_names(spec)
        out = np.empty((len(names), Z, Y, X), dtype=np.float32)
        self._ck(self._L.ekpnp_group_snapshot_read(self._g, C.byref(spec), out.ctypes.data_as(C.c_void_p)))
        return {n: out[i] for i, n in enumerate(names)}

    def save_checkpoint(self, path: str):
        self._ck(self._L.ekpnp_group_save_checkpoint(self._g, os.fsencode(path)))

    def load_checkpoint(self, path: str) -> float:
        t = C.c_double()
        self._ck(self._L.ekpnp_group_load_checkpoint(self._g, os.fsencode(path), C.byref(t)))
        return t.value
