"""What the CPU and the GPU tests of the tracer cloud's size thresholds share (tests/test_tracers_sizes_cpu.py, tests/test_tracers_sizes_gpu.py):
the particle counts and the level of each two-level kernel of csrc/tracers.hip they reach, and the builders of the clouds and tag lists
whose placement the GPU tests rely on.  Nothing here needs a device.

The tile sizes are not exported by the library.  CONSTANTS is what the source says today (the CPU file reads the source and compares);
`levels`, `cloud_bytes` and `sort_bytes` are the formulas ekpnp_device_bytes exposes them through, so that a change of a tile size
fails a test here instead of moving a size back below its threshold.

    kernel                                   level two begins at            sizes
    k_tracers_sort_scan / _scan_top /        a second chunk of TS_SCAN =    65 536 (16 runs: one chunk exactly full), 65 537 (17 runs, 2 chunks),
      _scatter                               4096 table entries = 16 runs   131 073 (33, 3), 1 048 577 (257 runs, 17 chunks)
    k_tracers_sort_scan_top's four waves     more than 64 chunks            4 194 305 (1025 runs, 65 chunks: one sum in the second wavefront)
    k_tracers_sort_scan_top's carry loop     more than 256 chunks           16 777 217 (4097 runs, 257 chunks)
    k_tracers_finish                         more than 16 partials          65 536 (16), 65 537 (17), 131 073 (33 = 16 + 16 + 1)
    k_tracers_cells<LDS> and <global>        a second workgroup of 8192     8192 (1 workgroup), 8193 (2), 24 653 (4), 65 537 (9)
    k_tracers_track_find                     n mod 4 != 0; ntags > 768      n = 4096 .. 4099 and 65 537 (65 workgroups); ntags = 257, 1024"""
import os
import re

import numpy as np

import _tracers_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "ek-pnp-3d_amd", "csrc", "tracers.hip")
SHAPES = {"R": (40, 12, 17), "T": (70, 66, 17), "W": (70, 66, 13)}
KEY_LOST = 0xFFFFFFFF

CONSTANTS = {"TR_THREADS": 256, "TR_PER_THREAD": 16, "TR_CELL_PER_THREAD": 32, "TR_LDS_CELLS": 8192, "TS_RUN": 4096, "TS_SCAN": 4096, "TK_IDS": 4}
FINISH_BATCH = 16      # partials k_tracers_finish loads per round (a literal in the kernel)
SCAN_TOP_ROUND = 256   # chunk sums k_tracers_sort_scan_top takes per round of its carry loop: TR_THREADS

# n -> what it reaches
SORT_NS = {65536: (16, 1), 65537: (17, 2), 131073: (33, 3), 1048577: (257, 17)}   # (runs, chunks)
WAVE_N = 4194305                                                                  # 1025 runs, 65 chunks: the second wavefront of the top scan
CARRY_N = 16777217                                                                # 4097 runs, 257 chunks: the second round of its carry loop
MOMENT_NS = {65536: 16, 65537: 17, 131073: 33}                                    # partials
CELL_NS = {8192: 1, 8193: 2, 3 * 8192 + 77: 4, 65537: 9}                          # workgroups of the cell counts
CELL_GRIDS = ((1, 1, 1), (16, 16, 12), (63, 13, 10), (64, 16, 8), (64, 64, 12))   # 8190 cells: the last grid in LDS; 8192: the first in global memory
TRACK_NS = (4096, 4097, 4098, 4099, 65537)
TRACK_NTAGS = (257, 1024)


def source_constants():
    """name -> value of every `constexpr int NAME = <number>;` of csrc/tracers.hip"""
    text = open(SOURCE, encoding="utf-8").read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^constexpr int (\w+) = (\d+);", text, re.M)}


def levels(n):
    """(nwg, nruns, chunks): workgroups of the moments' partials, runs of a sort pass, chunks of the scan of the digit table"""
    nwg = -(-n // (CONSTANTS["TR_THREADS"] * CONSTANTS["TR_PER_THREAD"]))
    nruns = -(-n // CONSTANTS["TS_RUN"])
    return nwg, nruns, -(-256 * nruns // CONSTANTS["TS_SCAN"])


def cloud_bytes(n, nwg):
    """six doubles and two int32 per particle, nwg rows of partial moments and the result"""
    return 56 * n + (nwg + 1) * 12 * 8


def sort_bytes(n, nruns, chunks):
    """the first sort: two item buffers, the digit table [256][nruns] and its chunk sums, and the ids"""
    return 16 * n + (256 * nruns + chunks) * 4 + 4 * n


def cell_workgroups(n):
    return -(-n // (CONSTANTS["TR_THREADS"] * CONSTANTS["TR_CELL_PER_THREAD"]))


def find_workgroups(n):
    return -(-n // (CONSTANTS["TR_THREADS"] * CONSTANTS["TK_IDS"]))


def keys(shape, x, y, z):
    """ekpnp_tracers_sort_key in numpy (the header's text, as tests/test_tracers_sort_cpu.py::keys_ref): uint32"""
    nx, ny, nz = shape
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    lost = np.isnan(x) | np.isnan(y) | np.isnan(z)
    xs, ys, zs = (np.where(lost, 0.0, a) for a in (x, y, z))
    i0, j0, k0 = xs.astype(np.int64), ys.astype(np.int64), np.minimum(zs.astype(np.int64), nz - 2)
    return np.where(lost, KEY_LOST, (k0 * ny + j0) * nx + i0).astype(np.uint32)


# ---- the clouds of the sort ------------------------------------------------------------------------------------------------------

def special_cloud(shape, n, seed):
    """T.special_cloud, and a lost particle in every run of 4096 and more (every 101st from slot 40 on)"""
    x, y, z = T.special_cloud(shape, n, seed)
    x[40::101] = y[40::101] = z[40::101] = np.nan
    return x, y, z


def sort_clouds(shape, n, seed):
    """the clouds of tests/test_tracers_sort_gpu.py::test_device_sort_equals_sort_host but the advanced one: name -> (x, y, z)"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    nodes = nx * ny * (nz - 1)
    k = (n - 1 - np.arange(n)) % nodes   # descending node index: memory order reversed (and, past `nodes` particles, equal keys far apart)
    nan = np.full(n, np.nan)
    return {
        "special": special_cloud(shape, n, seed),
        "reversed": ((k % nx) + 0.25, ((k // nx) % ny) + 0.5, (k // (nx * ny)) + 0.75),
        "one node": (3.0 + rng.uniform(0, 1, n), 5.0 + rng.uniform(0, 1, n), 2.0 + rng.uniform(0, 1, n)),
        "all lost": (nan, nan, nan),
    }


def spread_cloud(shape, n, seed, lost=1.0 / 64.0):
    """particle i in the middle of node (i * 2 654 435 761) mod nodes, a seeded fraction lost: keys spread over every byte a lattice has,
    neighbours in memory far apart in the lattice"""
    nx, ny, nz = shape
    nodes = nx * ny * (nz - 1)
    node = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761)) % np.uint64(nodes)   # (n < 2^28: the product stays below 2^60)
    node = node.astype(np.int64)
    x = (node % nx) + 0.5
    y = ((node // nx) % ny) + 0.5
    z = (node // (nx * ny)) + 0.5
    gone = np.random.default_rng(seed).random(n) < lost
    x[gone] = y[gone] = z[gone] = np.nan
    return x, y, z


# ---- the clouds of the moments ---------------------------------------------------------------------------------------------------

MOMENT_ROLES = ("lost", "z_min", "z_max")
MOMENT_U = (0.375 / 128.0, -0.25 / 128.0)   # with dx = dy = dz = 2^-17 and h = 2^-10: 3/8 and -1/4 of a cell per substep
MOMENT_NSUB = 8 * 40                        # 120 cells along x, -80 along y


def moment_roles(n):
    """the last workgroup of the partials holds slots 4096 (nwg - 1) .. n - 1.  With three slots or more it takes the lost particle,
    the unique z_min and the unique z_max at once; with fewer (65 537 and 131 073 leave it ONE slot) each of them takes the last slot
    in a cloud of its own"""
    first = 4096 * (levels(n)[0] - 1)
    return ("lost",) if n - first >= 3 else MOMENT_ROLES


def moments_cloud(shape, n, role, seed):
    """(x0, y0, z0, where): dyadic starts (multiples of 1/8; z in 1 .. nz-2, so the extremes below are unique).  Slot n - 1 holds `role`;
    slots n - 2 and n - 3 hold the other two where they still lie in the last workgroup of the partials.  At more than 16 partials
    one further particle is lost in the first slot of the second batch of k_tracers_finish (slot 16 * 4096; at 65 537 that IS slot
    n - 1).  where: name -> slot."""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    x0 = rng.integers(0, nx * 8, n) / 8.0
    y0 = rng.integers(0, ny * 8, n) / 8.0
    z0 = rng.integers(8, (nz - 2) * 8 + 1, n) / 8.0
    first = 4096 * (levels(n)[0] - 1)
    where = {}
    for k, r in enumerate((role, *[q for q in MOMENT_ROLES if q != role])):
        if n - 1 - k >= first:
            where[r] = n - 1 - k
    if levels(n)[0] > FINISH_BATCH and FINISH_BATCH * 4096 not in where.values():   # (at 65 537 that slot is the last one, taken by `role`)
        where["second batch"] = FINISH_BATCH * 4096
    for r, s in where.items():
        if r == "z_min":
            z0[s] = 0.125
        elif r == "z_max":
            z0[s] = nz - 1 - 0.125
        else:
            x0[s] = y0[s] = z0[s] = np.nan
    return x0, y0, z0, where


def moments_exact(n, z0):
    """the twelve moments after MOMENT_NSUB substeps of the uniform dyadic velocity, in integer arithmetic: every alive particle has
    moved 120 cells along x and -80 along y, none along z"""
    alive = ~np.isnan(z0)
    m = int(alive.sum())
    z8 = np.rint(z0[alive] * 8.0).astype(np.int64)
    assert np.array_equal(z8 / 8.0, z0[alive])
    return [float(m), float(n - m), 120.0 * m, -80.0 * m, 0.0, 14400.0 * m, 6400.0 * m, 0.0, int(z8.sum()) / 8.0, int((z8 * z8).sum()) / 64.0,
            int(z8.min()) / 8.0, int(z8.max()) / 8.0]


# ---- the cloud of the cell counts -------------------------------------------------------------------------------------------------

def cells_cloud(shape, n, seed):
    """T.special_cloud with about 1 % of the particles lost, in every workgroup's share"""
    x, y, z = T.special_cloud(shape, n, seed)
    gone = np.random.default_rng(seed + 1).random(n) < 0.01
    x[gone] = y[gone] = z[gone] = np.nan
    return x, y, z


# ---- the tag list of the tracks ---------------------------------------------------------------------------------------------------

TRACK_LOST = 12   # the particle of T.special_cloud that is lost from the start


def tag_list(n, ntags, must, seed):
    """ntags distinct ids in scrambled order that hold 0, n - 1, TRACK_LOST and every id of `must` (the ids a sort leaves in the
    last n mod 4 slots, which k_tracers_track_find reads one by one)"""
    need = list(dict.fromkeys([0, n - 1, TRACK_LOST, *[int(i) for i in must]]))
    assert len(need) <= ntags <= n
    rng = np.random.default_rng(seed)
    rest = rng.permutation(n)
    rest = rest[~np.isin(rest, need)][:ntags - len(need)]
    ids = np.concatenate([np.array(need, dtype=np.int64), rest.astype(np.int64)])
    return ids[rng.permutation(ntags)]


# ---- the large sorts: ids and x alone ---------------------------------------------------------------------------------------------

def large_sort_case(pkg, n, seed=5):
    """the spread cloud of n particles on lattice T, sorted on the device (needs one): the byte counts, ekpnp_tracers_ids against
    ekpnp_tracers_sort_host and x against x[perm].  Returns a record of what was held and the seconds each part took."""
    import time

    shape = SHAPES["T"]
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    nwg, nruns, chunks = levels(n)
    t = [time.perf_counter()]
    lap = lambda: t.append(time.perf_counter()) or round(t[-1] - t[-2], 3)
    x, y, z = spread_cloud(shape, n, seed)
    rec = {"n": n, "lattice": list(shape), "nruns": nruns, "chunks": chunks, "lost": int(np.isnan(x).sum()), "build_cloud_s": lap()}
    perm = pkg.tracers_sort_host(p, x, y, z)
    rec["sort_host_s"] = lap()
    with pkg.Solver(p) as s:
        empty = s.device_bytes()
        s.tracers_set(x, y, z)
        rec["cloud_bytes_as_the_formula"] = bool(s.device_bytes() == empty + cloud_bytes(n, nwg))
        rec["set_s"] = lap()
        s.tracers_sort()
        s.synchronize()
        rec["sort_bytes_as_the_formula"] = bool(s.device_bytes() == empty + cloud_bytes(n, nwg) + sort_bytes(n, nruns, chunks))
        rec["device_bytes"] = int(s.device_bytes() - empty)
        rec["device_sort_s"] = lap()
        ids = s.tracers_ids()
        got = s.tracers_get()[0]
        rec["read_back_s"] = lap()
    rec["ids_equal_sort_host"] = bool(np.array_equal(ids, perm))
    rec["x_equals_x_of_perm"] = bool(T.same(got, x[perm]))
    rec["moved"] = int((perm != np.arange(n, dtype=perm.dtype)).sum())
    rec["compare_s"] = lap()
    rec["total_s"] = round(t[-1] - t[0], 3)
    return rec
