"""What the CPU and the GPU tests of the field diagnostics' size thresholds share (tests/test_diag_sizes_cpu.py,
tests/test_diag_sizes_gpu.py): the lattice shapes and the path of each kernel of csrc/{stats,monitor,modes,hist,diag,section,spectrum,
snapshot}.hip they reach, the builders of the fields whose placements the GPU tests rely on, and the host references.  Nothing here
needs a device.

The tile sizes are not exported by the library.  CONSTANTS is what the sources say today (the CPU file reads the sources and compares);
the workgroup counts and byte counts below are the formulas of the need_* functions, through which ekpnp_device_bytes exposes them, so
that a retuned tile size fails a test here instead of moving a shape back below its threshold.

    kernel                                      path                                                  first reached at    shapes
    k_monitor_planes, k_mode_finish             second batch of 16 workgroup partials (4096 nodes)    plane > 65 536      A (16, the last before), B (17), C (33), D (65)
    k_hist_finish                               second batch of 8 count tables (8192 nodes)           plane > 65 536      A (8), B (9), C (17), D (33)
    k_hist_partials / hist_chunk                chunks of 16 384 and 24 576 nodes, 2 .. 12 tiles      plane >= the chunk  C, D with 2048 / 4096 / 64 x 64 bins
    k_range_finish                              a lane's second round over 64 partials of 4096        plane > 262 144     D (65 partials)
    k_monitor_plates, k_wall_current, k_max_uz  grid-stride second round of 1024 blocks of 256        > 262 144 nodes     D (plane); B, C, D (k_max_uz: nodes of the context)
    k_final, plate part of k_monitor_finish     a thread's second round over 256 partials             plane > 65 536      B (257 partials), C, D
    k_monitor_finish, volume part               plane results from global memory, not LDS             586 planes          E585 (4095 doubles in LDS), E586
    k_section_y                                 a second workgroup of 256 along x                     nx > 256            B, C, D
    k_section_x                                 more than two row tiles, more than three runs         ny > 128, nx > 192  C (7 / 13 tiles, 6 runs), D
    spectrum plan                               a batch of fewer than 16 planes                       > 4 MiB a plane     F (15 + 1)
    k_snapshot                                  more than two x chunks per output row                 nx / cx > 128       C (6 chunks)
k_plane_partials / k_plane_finish (stats.hip) have no second level and ride along on the same shapes.

Fields.  `dyadic_fields`: signed integers in [-1024, 1024] times 2^-10 (rho: 1000 plus that), so that every sum of terms and of
products of two terms is exact in float64 IN ANY ORDER and the device must return the exact sum, computed here in int64, with ==.
`random_fields`: arbitrary float64, for everything that has a host definition (sections, histogram counts, value ranges, snapshots).

The references that other test files already define are taken from there, not copied: the snapshot's block means
(tests/test_snapshot_gpu.py::_ref), the phases of a mode (tests/test_modes_gpu.py::_phase), the histogram index and counts in numpy
(tests/test_hist_gpu.py::_index, ::_counts), the peak's tie rule (tests/test_spectrum_gpu.py::_numpy_peak) and the energies of a modes
row (tests/_observer_pairs.py::energies)."""
import ctypes as C
import os
import re

import numpy as np

from _observer_pairs import energies                     # noqa: F401  (re-exported)
from test_hist_gpu import _counts as hist_counts         # noqa: F401
from test_hist_gpu import _index as hist_index           # noqa: F401
from test_modes_gpu import _phase as mode_phase          # noqa: F401
from test_snapshot_gpu import _ref as snapshot_ref       # noqa: F401
from test_spectrum_gpu import _numpy_peak as spectrum_peak   # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ek-pnp-3d_amd", "csrc")
HEADER = os.path.join(ROOT, "include", "ekpnp.h")

# (nx, ny, nz).  E: the library accepts nx = 16, ny = 4 (ekpnp_create asks for 1 x 1 x 4 at least).  S: C's plane in nine planes, the
# fewest a group of two UNEVEN slabs can have (a slab needs four planes: 4 + 5).  F: nz = 16 is the fewest planes that give two batches.
SHAPES = {"A": (256, 256, 4), "B": (257, 256, 4), "C": (331, 397, 4), "D": (520, 505, 4), "E585": (16, 4, 585), "E586": (16, 4, 586),
          "F": (1024, 512, 16), "S": (331, 397, 9)}

# file -> name -> value, as the sources have them today
CONSTANTS = {
    "stats.hip": {"STATS_THREADS": 256, "STATS_PER_THREAD": 16, "STATS_CHUNK": 4096},
    "monitor.hip": {"MON_THREADS": 256, "MON_PER_THREAD": 16, "MON_CHUNK": 4096, "MON_PLATE_BLOCKS": 1024, "MON_NV": 7, "MON_NVSUM": 5, "MON_LDS_PLANES": 4096},
    "modes.hip": {"MODE_THREADS": 256, "MODE_PER_THREAD": 16, "MODE_CHUNK": 4096},
    "hist.hip": {"HIST_THREADS": 256, "HIST_LOADS": 16, "HIST_CHUNK0": 8192},
    "diag.hip": {"DIAG_BLOCKS": 1024},
    "section.hip": {"SEC_RUN": 64, "SEC_Y_THREADS": 256, "SEC_X_LOADS": 16},
    "spectrum.hip": {"SPEC_BATCH_BYTES": 64 << 20},
    "snapshot.hip": {"SNAP_LANES": 64},
    "ekpnp.h": {"EKPNP_MAX_SPECTRUM_PLANES": 16, "EKPNP_MAX_MODES": 16, "EKPNP_HIST_MAX_BINS": 4096, "EKPNP_NMONITORS": 11, "EKPNP_NPROFILES": 24},
}
K = {k: v for d in CONSTANTS.values() for k, v in d.items()}
FINISH_BATCH = 16   # partials k_monitor_planes and k_mode_finish load per round (a literal in the kernels)
HIST_BATCH = 8      # count tables k_hist_finish loads per round (a literal)
FINAL_THREADS = 256  # threads of k_final and k_monitor_finish: partials per round
RANGE_LANES = 64    # lanes of k_range_finish: partials per round
SEC_X_ROWS = (64, 32)   # rows of a tile of k_section_x: one array, the pair c / cn


def source_constants(name):
    """name -> value of every `constexpr <int | long long | size_t> NAME = <expression of numbers and earlier names>;` of csrc/<name>, or
    of every `#define EKPNP_X <number>` and `EKPNP_X = <number>` of the header"""
    if name == "ekpnp.h":
        text = open(HEADER, encoding="utf-8").read()
        out = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (EKPNP_\w+) (\d+)\s*$", text, re.M)}
        out.update({m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*(EKPNP_N\w+) = (\d+)\s*$", text, re.M)})
        return out
    text = open(os.path.join(CSRC, name), encoding="utf-8").read()
    out = {}
    for m in re.finditer(r"^constexpr (?:int|long long|size_t) (\w+) = ([^;]+);", text, re.M):
        expr = m.group(2).replace("(size_t)", "")
        if re.fullmatch(r"[\w\s*+<>()-]+", expr) and all(t.isdigit() or t in out for t in re.findall(r"\w+", expr)):
            out[m.group(1)] = int(eval(expr, {"__builtins__": {}}, dict(out)))   # numbers, earlier constants, * + - << only
    return out


# ---- the counts of the table above, by the formulas of the sources ----------------------------------------------------------------

def plane(shape):
    return shape[0] * shape[1]


def ceil_div(a, b):
    return -(-a // b)


def chunk_workgroups(shape):
    """workgroups per plane of k_plane_partials, k_monitor_volume, k_mode_partials (stats_workgroups_per_plane, mon_workgroups, mode_workgroups)"""
    return ceil_div(plane(shape), K["STATS_CHUNK"])


def plate_blocks(n):
    """blocks of k_monitor_plates / k_wall_current over a plane of n nodes, of k_max_uz over n nodes (mon_plate_blocks, launch_current, launch_umax)"""
    return min(ceil_div(n, 256), K["MON_PLATE_BLOCKS"])


def hist_stride(a, b=None):
    """cells + 1 of a spec: (a.n + 2) (b.n + 2), and the nonfinite counter"""
    return (a[1] + 2) * ((b[1] + 2) if b else 1) + 1


def hist_chunk(stride):
    """hist_chunk_nodes: nodes of a plane per workgroup"""
    return K["HIST_CHUNK0"] * ceil_div(stride, 2048)


def hist_workgroups(shape, stride):
    return ceil_div(plane(shape), hist_chunk(stride))


def hist_tiles(stride, narr, vec):
    """tiles of a full chunk in hist_chunk<..., VEC>: L loads of VEC doubles per thread and array"""
    loads = {1: K["HIST_LOADS"], 2: K["HIST_LOADS"] // 2, 3: K["HIST_LOADS"] // 4, 4: K["HIST_LOADS"] // 4}[narr]
    return ceil_div(hist_chunk(stride), K["HIST_THREADS"] * loads * vec)


def range_workgroups(shape):
    return ceil_div(plane(shape), K["HIST_THREADS"] * K["HIST_LOADS"])


def spectrum_batch(shape):
    """SpecState::B of need_spectrum"""
    per_plane = shape[1] * (shape[0] // 2 + 1) * 16
    return max(1, min(K["SPEC_BATCH_BYTES"] // per_plane, K["EKPNP_MAX_SPECTRUM_PLANES"]))


# bytes a first call adds to ekpnp_device_bytes (nzl planes in the context)
def stats_bytes(shape, nzl):
    """need_stats: [partials | sums of the last pass | running sums]"""
    return (nzl * chunk_workgroups(shape) * K["EKPNP_NPROFILES"] + 2 * K["EKPNP_NPROFILES"] * nzl) * 8


def monitor_bytes(shape, nzl):
    """need_monitor: [plate partials | volume partials | plane results | one row]"""
    return (4 * K["MON_PLATE_BLOCKS"] + nzl * chunk_workgroups(shape) * K["MON_NV"] + nzl * K["MON_NV"] + 16) * 8


def modes_bytes(shape, nzl):
    """need_modes: [partials | (a, b) | two table slots of EKPNP_MAX_MODES (nx + ny) (cos, sin) pairs]"""
    m = K["EKPNP_MAX_MODES"]
    return (nzl * chunk_workgroups(shape) * 2 * m + m * nzl * 2 + 2 * 2 * m * (shape[0] + shape[1])) * 8


def hist_bytes(shape, nzl, strides, ranges=False):
    """hist_scratch after passes with these strides (and a value_range): both buffers grow to the largest asked for"""
    part = max([nzl * hist_workgroups(shape, s) * s * 4 for s in strides] + ([nzl * range_workgroups(shape) * 16] if ranges else []))
    planes = max([nzl * s * 8 for s in strides] + ([nzl * 16] if ranges else []))
    return part + planes


def spectrum_buffer_bytes(shape, nzl, nshell):
    """need_spectrum's own buffer (the transform's work area comes on top): B spectra, B staged planes, the result rows, the shell table"""
    nx, ny, _ = shape
    even = lambda n: (n + 1) & ~1
    B, nspec = spectrum_batch(shape), ny * (nx // 2 + 1)
    rows = max(nzl, K["EKPNP_MAX_SPECTRUM_PLANES"])
    return (2 * B * nspec + even(B * nx * ny) + even(rows * (nshell + 3))) * 8 + (nshell + 1 + nspec) * 4


# ---- fields -------------------------------------------------------------------------------------------------------------------------

FIELDS = ["rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T"]
PROFILES = FIELDS + ["ux_ux", "uy_uy", "uz_uz", "c_c", "cn_cn", "T_T", "uz_T", "uz_c", "uz_cn", "q_Ex", "q_Ez", "ux_uz", "q_q"]
RHO0 = 1000.0        # ekpnp_default_params; a dyadic number (the CPU file holds it against the library's)
Q = 1024             # the grid of the dyadic fields: 2^-10
PLANT_UZ = 2.0       # the unique largest uz: every other one is at most 1
PLANT_RHO = 2.0      # rho - rho0 of the unique largest |rho - rho0|


def plants(shape):
    """name -> (z, node of the plane): the nodes a broken second level would lose, as far as the shape has them.
    last: the last live node of the last workgroup of the last plane - the last node k_max_uz reads, in its last grid-stride round
    (node index of the context >= 262 144 from B on; on D the plane index is too); on E586 the plane above the 585 that fit LDS;
    batch2: the first node of workgroup 16, the first the second batch of k_monitor_planes / k_mode_finish holds (plane > 65 536)"""
    nx, ny, nz = shape
    P = nx * ny
    out = {"last": (nz - 1, P - 1)}
    if P > FINISH_BATCH * K["MON_CHUNK"]:
        out["batch2"] = (nz - 2, FINISH_BATCH * K["MON_CHUNK"])
    return out


def dyadic_fields(shape, seed, variant=0, nan=None, names=FIELDS):
    """name -> [nz][ny][nx]: integers in [-1024, 1024] times 2^-10, a seed per field (rho: RHO0 plus that).  The unique largest uz
    (PLANT_UZ) and the unique largest |rho - rho0| (PLANT_RHO) sit at two different nodes of plants(shape): variant 0 puts uz at "last"
    and rho at "batch2" (or, without one, at the last node of plane 1); variant 1 swaps them.  nan: a (z, node) at which c is NaN."""
    nx, ny, nz = shape
    P = nx * ny
    f = {}
    for name in names:
        rng = np.random.default_rng(1000 * seed + FIELDS.index(name))
        f[name] = rng.integers(-Q, Q + 1, size=(nz, ny, nx)).astype(np.float64) / Q
    pl = plants(shape)
    a, b = pl["last"], pl.get("batch2", (1, P - 1))
    if variant:
        a, b = b, a
    if "uz" in f:
        f["uz"].reshape(nz, P)[a] = PLANT_UZ
    if "rho" in f:
        f["rho"] += RHO0
        f["rho"].reshape(nz, P)[b] = RHO0 + PLANT_RHO
    if nan is not None:
        f["c"].reshape(nz, P)[nan] = np.nan
    return f


def random_fields(shape, seed):
    """arbitrary float64 fields of the magnitudes of a perturbed run (the scales of the other diagnostics tests), and for value_range
    the unique smallest uz and q at the last node of every plane (the last partial of k_range_partials) and the unique largest at the
    first node of partial 64 (plane > 262 144: the second round of k_range_finish's lanes), else of partial 16, else at node 1"""
    nx, ny, nz = shape
    P = nx * ny
    rng = np.random.default_rng(seed)
    scale = {"rho": 1000.0, "c": 30.0, "cn": 30.0, "phi": 5e-3, "T": 1.0, "Ex": 1e5, "Ey": 1e5, "Ez": 1e5}
    f = {n: scale.get(n, 1e-3) * rng.uniform(-1.0, 1.0, size=(nz, ny, nx)) for n in FIELDS}
    top = range_top_node(shape)
    for z in range(nz):
        for name, v in (("uz", 2e-3 + 1e-5 * z), ("c", 40.0 + z)):
            f[name].reshape(nz, P)[z, P - 1] = -v
            f[name].reshape(nz, P)[z, top] = v
        f["cn"].reshape(nz, P)[z, P - 1] = 40.0
        f["cn"].reshape(nz, P)[z, top] = -40.0
    return f


def range_top_node(shape):
    P = plane(shape)
    per = K["HIST_THREADS"] * K["HIST_LOADS"]
    return RANGE_LANES * per if P > RANGE_LANES * per else (16 * per if P > 16 * per else 1)


def nan_node(shape):
    """where the twin's c is NaN: the last live node of the last workgroup - of the plane next to the upper plate where the context has
    four planes (both plates read it: the currents are NaN too), of the last plane otherwise (E586: the plane above the 585 in LDS)"""
    nx, ny, nz = shape
    return (nz - 2 if nz == 4 else nz - 1, nx * ny - 1)


# name -> (axis a, axis b or None, arrays read): the ranges lie inside what random_fields spreads, so both outer cells fill
HIST_SPECS = {
    "uz128": (("uz", 128, -0.9e-3, 0.8e-3), None, 1),                                # stride 131: chunk 8192
    "T2048": (("T", 2048, -0.6, 0.8), None, 1),                                      # stride 2051: chunk 16 384
    "q4096": (("q", 4096, -25.0, 31.5), None, 2),                                    # stride 4099: chunk 24 576
    "q_uz": (("q", 64, -25.0, 31.5), ("uz", 64, -0.9e-3, 0.8e-3), 3),                # stride 4357: chunk 24 576, three arrays
    "uz_T": (("uz", 32, -0.5e-3, 0.7e-3), ("T", 32, -0.6, 0.8), 2),                  # stride 1157: chunk 8192, no q
}


# ---- exact references of the dyadic fields: int64 ---------------------------------------------------------------------------------

def to_int(a):
    """the integers of a dyadic array (a NaN as 0), and that the array is on the grid"""
    bad = np.isnan(a)
    i = np.rint(np.where(bad, 0.0, a) * Q).astype(np.int64)
    assert np.array_equal(np.where(bad, 0.0, a), i / float(Q))
    return i


def _exact(total, nan, quanta):
    """an int64 sum of numbers on the grid 1 / quanta as a float64 (exact: |total| < 2^53), or NaN where a term was"""
    total = np.asarray(total)
    assert (np.abs(total) < 2 ** 53).all()
    return np.where(nan, np.nan, total.astype(np.float64) / float(quanta))


def plane_sums_exact(f):
    """[24][nz]: the sums of ekpnp_plane_sums (stats.hip's k_plane_partials: the eleven fields, then the thirteen products in the order
    of the EKPNP_PROF_* ids), NaN where a NaN enters"""
    i = {n: to_int(f[n]) for n in FIELDS}
    bad = {n: np.isnan(f[n]) for n in FIELDS}
    i["q"], bad["q"] = i["c"] - i["cn"], bad["c"] | bad["cn"]
    ax = (1, 2)
    rows = [_exact(i[n].sum(axis=ax), bad[n].any(axis=ax), Q) for n in FIELDS]
    for name in PROFILES[len(FIELDS):]:
        a, b = name.split("_")
        rows.append(_exact((i[a] * i[b]).sum(axis=ax), (bad[a] | bad[b]).any(axis=ax), Q * Q))
    return np.array(rows)


def monitor_exact(f, p, top=True, bottom=True):
    """the eleven scalars of a monitor row of a context that holds the planes of f (monitor.hip).  The plate sums are those of
    k_monitor_plates: (2 c(n1) - c(n2) - (2 cn(n1) - cn(n2))) Ez(w) and 3 T(w) - 4 T(n1) + T(n2) (upper plate; the lower one
    4 T(n1) - 3 T(w) - T(n2)), w the plate, n1 and n2 the planes next to it; k_monitor_finish scales a current as r * K * dz * dz,
    left to right (its lines `row[0] = r * a.K * a.dz * a.dz`, the expression of ekpnp_current in io.hip), and stores the wall
    gradients as they are.  The volume sums are k_monitor_volume's: ux ux + uy uy + uz uz, q, q q, uz T with q = c - cn; uz_max
    starts at 0; rho_dev = max |rho - rho0|, one FP64 subtraction per node; nonfinite counts the nodes where rho, c, cn or T is not
    finite.  A sum a NaN enters is NaN; fmax drops it."""
    i = {n: to_int(f[n]) for n in FIELDS}
    bad = {n: np.isnan(f[n]) for n in FIELDS}
    out = np.zeros(11)

    def plate(w, n1, n2, sign):
        cur = ((2 * i["c"][n1] - i["c"][n2]) - (2 * i["cn"][n1] - i["cn"][n2])) * i["Ez"][w]
        cur_bad = bad["c"][n1] | bad["c"][n2] | bad["cn"][n1] | bad["cn"][n2] | bad["Ez"][w]
        grad = sign * (3 * i["T"][w] - 4 * i["T"][n1] + i["T"][n2])
        grad_bad = bad["T"][w] | bad["T"][n1] | bad["T"][n2]
        r = float(_exact(cur.sum(), cur_bad.any(), Q * Q))
        return r * p.K * p.dz * p.dz, float(_exact(grad.sum(), grad_bad.any(), Q))

    if top:
        out[0], out[3] = plate(-1, -2, -3, 1)
    if bottom:
        out[1], out[2] = plate(0, 1, 2, -1)
    q, qbad = i["c"] - i["cn"], bad["c"] | bad["cn"]
    ubad = bad["ux"] | bad["uy"] | bad["uz"]
    out[4] = max(0.0, float(np.nanmax(f["uz"])))
    out[5] = _exact((i["ux"] * i["ux"] + i["uy"] * i["uy"] + i["uz"] * i["uz"]).sum(), ubad.any(), Q * Q)
    out[6] = _exact(q.sum(), qbad.any(), Q)
    out[7] = _exact((q * q).sum(), qbad.any(), Q * Q)
    out[8] = _exact((i["uz"] * i["T"]).sum(), (bad["uz"] | bad["T"]).any(), Q * Q)
    out[9] = float(np.nanmax(np.abs(f["rho"] - p.rho0)))
    out[10] = float((~(np.isfinite(f["rho"]) & np.isfinite(f["c"]) & np.isfinite(f["cn"]) & np.isfinite(f["T"]))).sum())
    return out


def worst_case_quanta(shape):
    """the largest |sum| any test forms over a plane of dyadic fields, in quanta of 2^-20: a wall-current term is at most
    (2 + 1 + 2 + 1) * 1, rho rho0-sized, the planted values 2, and the running sums hold two passes"""
    P = plane(shape)
    term = max(6 * Q * Q, int(RHO0 + PLANT_RHO) * Q * Q, 3 * (int(PLANT_UZ) * Q) ** 2)
    return 2 * P * term


# ---- references with a host definition --------------------------------------------------------------------------------------------

def value(f, name):
    return f["c"] - f["cn"] if name == "q" else f[name]   # one FP64 subtraction per node, before anything else


def section_ref(pkg, v, across, lo, hi):
    """[nz][nkeep]: ekpnp_section_sum of every line of v ([nz][ny][nx], contiguous) summed along `across` over lo .. hi"""
    v = np.ascontiguousarray(v, dtype=np.float64)
    nz, ny, nx = v.shape
    fn = pkg.load_library().ekpnp_section_sum
    base, n = v.ctypes.data, hi - lo + 1
    if across == "x":
        nkeep, first, step, stride = ny, lo, nx, 1
    else:
        nkeep, first, step, stride = nx, lo * nx, 1, nx
    out = np.empty((nz, nkeep))
    for z in range(nz):
        at = base + 8 * (z * ny * nx + first)
        out[z] = [fn(C.c_void_p(at + 8 * k * step), stride, n) for k in range(nkeep)]
    return out


def section_ranges(shape, across):
    """full; lo == hi (a cut: the field's own bits); one that starts at an odd index and ends inside a run (3 .. n - 30: more than two runs)"""
    n = shape[0] if across == "x" else shape[1]
    return {"full": (0, n - 1), "cut": (n // 2, n // 2), "odd": (3, n - 30)}


def rfft2_power(v):
    """P[ny][nx/2 + 1] of include/ekpnp.h from numpy's rfft2: w (re^2 + im^2), w = 1 for m = 0 and the even Nyquist column, else 2"""
    F = np.fft.rfft2(v)
    w = np.full(F.shape[1], 2.0)
    w[0] = 1.0
    if v.shape[1] % 2 == 0:
        w[-1] = 1.0
    return w[None, :] * (F.real * F.real + F.imag * F.imag)


def power_tolerance(v):
    """4 u, u = log2(nx ny) 2^-53 nx ny sum v^2: the bound of tests/test_spectrum_gpu.py::test_powers_against_the_exact_transform_and_parseval
    (its _u; 4 u is what it allows at every shape), the sum of squares exact in int64 for a dyadic plane instead of in Fractions"""
    ny, nx = v.shape
    i = to_int(v)
    s2 = int((i * i).sum())
    assert s2 < 2 ** 53
    return 4.0 * np.log2(nx * ny) * 2.0 ** -53 * nx * ny * (s2 / float(Q * Q))


def mode_bound(v):
    """(nx ny + 16) 2^-53 sum |v|: the bound of tests/test_modes_gpu.py::test_amplitudes_against_fsum_of_the_double_products on |gpu - fsum|"""
    import math

    return (v.size + 16) * 2.0 ** -53 * math.fsum(np.abs(v).ravel().tolist())


def modes_of(shape):
    """sixteen modes: (0, 0), (1, 0), the largest m with the most negative n, and thirteen more over both signs of n"""
    nx, ny, _ = shape
    top = (nx // 2, -((ny - 1) // 2))
    more = [(0, 1), (1, 1), (1, -1), (2, 3), (3, -2), (5, 0), (0, ny // 2), (nx // 2, 0), (7, 11), (13, -17), (64, 64), (100, -100), (nx // 2 - 1, ny // 2 - 1)]
    return [(0, 0), (1, 0), top] + more
