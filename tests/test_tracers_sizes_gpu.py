"""GPU tests of the tracer cloud past every size threshold of its kernels (csrc/tracers.hip).  The other tracer tests run at n <= 12 365,
where each two-level kernel runs its first level only: one chunk of the digit table's scan, one batch of the moments' partials, one
workgroup of the cell counts.  Here n is chosen per kernel so that the second level runs (tests/_tracers_sizes.py holds the table;
tests/test_tracers_sizes_cpu.py holds the sizes against the constants of the source and the cloud builders to their placements), and
the byte counts of ekpnp_device_bytes show, per size, the workgroups, runs and chunks that were reached.

As in the other tracer tests the host functions are the definitions and the device is compared with them EXACTLY: arrays on their
float64 bit patterns, ids and counts as integers, the moments of dyadic displacements with ==.  The one tolerance is the a-priori bound
n * 2^-53 * sum|term| of tests/test_tracers_gpu.py on the sums of random displacements.  Lattices R 40 x 12 x 17, T 70 x 66 x 17 (two
values of the third key byte, and the lost particles give the fourth two) and, for the cell counts, W 70 x 66 x 13."""
import math

import numpy as np
import pytest

import _tracers_ref as T
import _tracers_sample_ref as S
import _tracers_sizes as Z

pytestmark = pytest.mark.gpu
UE = ("ux", "uy", "uz", "Ex", "Ey", "Ez")
ARRAYS = ("x", "y", "z", "x0", "y0", "z0", "wx", "wy")
BY_FILE = 200000   # up to here all eight arrays are read through the cloud's file, above it five through ekpnp_tracers_get


def _params(pkg, shape):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    return p


@pytest.fixture(scope="module")
def inputs():
    """per lattice: (u, E) random fields; made once, never modified"""
    out = {}
    for k, s in Z.SHAPES.items():
        u, E = T.random_fields(s, 281 + len(out), T.U_SCALE, T.E_SCALE)
        for a in (*u, *E):
            a.setflags(write=False)
        out[k] = (u, E)
    return out


def _put_fields(s, u, E):
    for name, a in zip(UE, (*u, *E)):
        s.set_field(name, a)


def _parse(raw):
    """the cloud's file: ({x, y, z, x0, y0, z0, wx, wy}, ids or None)"""
    assert raw[:8] == b"EKPNPTR1"
    reserved = int(np.frombuffer(raw[20:24], dtype="<i4")[0])
    n = int(np.frombuffer(raw[24:32], dtype="<i8")[0])
    assert len(raw) == 48 + (60 if reserved == 1 else 56) * n, (len(raw), reserved, n)
    d = np.frombuffer(raw[48:48 + 48 * n], dtype="<f8").reshape(6, n)
    w = np.frombuffer(raw[48 + 48 * n:48 + 56 * n], dtype="<i4").reshape(2, n)
    return dict(zip(ARRAYS, [*d, *w])), (np.frombuffer(raw[48 + 56 * n:], dtype="<i4") if reserved == 1 else None)


def _read(s, path):
    """the cloud in slot order: all eight arrays from its file, or (large clouds) the five of ekpnp_tracers_get"""
    if s.tracers_size > BY_FILE:
        return dict(zip(("x", "y", "z", "wx", "wy"), s.tracers_get()))
    s.tracers_save(str(path), time=0.5)
    cloud, ids = _parse(open(path, "rb").read())
    assert ids is None or np.array_equal(ids, s.tracers_ids())
    return cloud


def _assert_permuted(after, before, perm, what):
    assert set(after) == set(before) and len(after) >= 5
    for name, a in after.items():
        want = before[name][perm]
        assert a.dtype == want.dtype and (T.same(a, want) if a.dtype == np.float64 else np.array_equal(a, want)), (what, name)


def _assert_sorted(pkg, shape, cloud, what):
    keys = Z.keys(shape, cloud["x"], cloud["y"], cloud["z"]).astype(np.int64)
    assert (np.diff(keys) >= 0).all(), what
    assert (keys[-1] == pkg.TRACERS_KEY_LOST) == bool(np.isnan(cloud["x"]).any()), what
    return keys


# ---- 0 and 1. the sort past one chunk of the scan ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(Z.SORT_NS))
def test_device_sort_equals_sort_host_past_one_chunk(pkg, inputs, n, tmp_path):
    nruns, chunks = Z.SORT_NS[n]
    assert Z.levels(n) == (nruns, nruns, chunks)
    shape = Z.SHAPES["T"]
    u, E = inputs["T"]
    p = _params(pkg, shape)
    path = tmp_path / "cloud.bin"
    clouds = Z.sort_clouds(shape, n, 300 + n)
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        empty = s.device_bytes()
        for name, (x, y, z) in clouds.items():
            s.tracers_set(x, y, z)
            if name == "special":
                assert s.device_bytes() == empty + 56 * n + (nruns + 1) * 12 * 8, (n, "nwg", nruns)
            assert np.array_equal(s.tracers_ids(), np.arange(n))
            before = _read(s, path)
            assert T.same(before["x"], x) and not before["wx"].any()
            perm = pkg.tracers_sort_host(p, x, y, z)
            s.tracers_sort()
            if name == "special":   # the first sort of this context: the digit table of nruns runs and its chunk sums
                assert s.device_bytes() == empty + 56 * n + (nruns + 1) * 96 + 16 * n + (256 * nruns + chunks) * 4 + 4 * n, (n, nruns, chunks)
            assert np.array_equal(s.tracers_ids(), perm), (n, name)
            after = _read(s, path)
            _assert_permuted(after, before, perm, (n, name))
            keys = _assert_sorted(pkg, shape, after, (n, name))
            if name in ("one node", "all lost"):
                assert np.array_equal(perm, np.arange(n))
            else:
                assert (perm != np.arange(n)).sum() > n // 2
            if name == "special":   # every pass saw more than one digit
                assert all(len(set((keys >> (8 * b)) & 255)) > 1 for b in range(4))
        assert s.device_bytes() == empty + Z.cloud_bytes(n, nruns) + Z.sort_bytes(n, nruns, chunks)   # nothing grew with the later sorts
        # a cloud already advanced with a mobility: wx, wy are non-zero and the start differs from the position
        x, y, z = clouds["special"]
        s.tracers_set(x, y, z)
        s.tracers_advance(T.substep(p), nsub=7, mu=T.MU)
        before = _read(s, path)
        assert before["wx"].any() and before["wy"].any() and not T.same(before["x"], x) and np.isnan(before["x"]).any()
        if "x0" in before:
            assert T.same(before["x0"], x)
        perm = pkg.tracers_sort_host(p, before["x"], before["y"], before["z"])
        s.tracers_sort()
        assert np.array_equal(s.tracers_ids(), perm), (n, "advanced")
        after = _read(s, path)
        _assert_permuted(after, before, perm, (n, "advanced"))
        keys = _assert_sorted(pkg, shape, after, (n, "advanced"))
        assert all(len(set((keys >> (8 * b)) & 255)) > 1 for b in range(4))


def test_sorting_changes_no_trajectory_and_sorts_compose_at_33_runs(pkg, inputs, tmp_path):
    n = 131073
    assert Z.levels(n) == (33, 33, 3)
    shape = Z.SHAPES["T"]
    u, E = inputs["T"]
    p = _params(pkg, shape)
    path = tmp_path / "cloud.bin"
    x, y, z = Z.special_cloud(shape, n, 400 + n)
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        for s in (a, b):
            _put_fields(s, u, E)
            s.tracers_set(x, y, z)
        a.tracers_sort()
        for s in (a, b):
            s.tracers_advance(T.substep(p), nsub=7, mu=T.MU)
        ids1 = a.tracers_ids()
        assert not np.array_equal(ids1, np.arange(n))
        got, want = a.tracers_get(by_id=True), b.tracers_get()
        for k, name in enumerate(("x", "y", "z")):
            assert T.same(got[k], want[k]), name
        assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
        assert want[3].any() and np.isnan(want[0]).any() and not T.same(a.tracers_get()[0], want[0])   # the slots really moved
        # the moved cloud sorted again: the ids compose
        moved = _read(a, path)
        perm2 = pkg.tracers_sort_host(p, moved["x"], moved["y"], moved["z"])
        assert (perm2 != np.arange(n)).sum() > n // 2
        a.tracers_sort()
        third = _read(a, path)
        assert np.array_equal(a.tracers_ids(), ids1[perm2])
        _assert_permuted(third, moved, perm2, "second sort")
        # and a sort of the sorted cloud leaves every slot where it is
        a.tracers_sort()
        fourth = _read(a, path)
        assert np.array_equal(a.tracers_ids(), ids1[perm2])
        _assert_permuted(fourth, third, np.arange(n), "third sort")
        back = a.tracers_get(by_id=True)
        assert all(T.same(back[k], want[k]) for k in range(3)) and np.array_equal(back[3], want[3])


# ---- 2. the four waves and the carry loop of k_tracers_sort_scan_top ---------------------------------------------------------------

def _assert_large_sort(rec, runs, chunks):
    print(rec)
    assert (rec["nruns"], rec["chunks"]) == (runs, chunks)
    assert rec["cloud_bytes_as_the_formula"] and rec["sort_bytes_as_the_formula"]
    assert rec["lost"] > rec["n"] // 128 and rec["moved"] > rec["n"] // 2
    assert rec["ids_equal_sort_host"] and rec["x_equals_x_of_perm"]


def test_sort_with_a_chunk_sum_in_the_second_wavefront_of_the_top_scan(pkg):
    """4 194 305 particles: 1025 runs and 65 chunk sums, one more than a wavefront of k_tracers_sort_scan_top holds; ids and x alone"""
    _assert_large_sort(Z.large_sort_case(pkg, Z.WAVE_N), 1025, 65)


def test_sort_with_a_second_round_of_the_carry_loop(pkg):
    """16 777 217 particles: 4097 runs and 257 chunk sums, the second round of the carry loop of k_tracers_sort_scan_top holds one
    live sum; ids and x alone (1.28 GB on the device, 0.5 GB on the host).  Measured on one MI355X: 1.6 s inside the suite - the cloud
    0.27 s, the std::sort of the definition 0.97 s, set and upload 0.05 s, the device sort 4 ms, read back 0.05 s, the comparison 0.18 s -
    and 5.5 s as the first test of a process (the first use of the device); under 10 s, so it stays in the suite"""
    _assert_large_sort(Z.large_sort_case(pkg, Z.CARRY_N), 4097, 257)


# ---- 3. the moments past one batch of k_tracers_finish ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(Z.MOMENT_NS))
def test_moments_are_exact_on_dyadic_displacements_past_16_partials(pkg, n):
    nwg = Z.MOMENT_NS[n]
    assert Z.levels(n)[0] == nwg
    shape = Z.SHAPES["R"]
    nx, ny, nz = shape
    p = _params(pkg, shape)
    p.dx = p.dy = p.dz = 2.0 ** -17
    u = [np.full((nz, ny, nx), Z.MOMENT_U[0]), np.full((nz, ny, nx), Z.MOMENT_U[1]), np.zeros((nz, ny, nx))]
    with pkg.Solver(p) as s:
        _put_fields(s, u, [np.zeros((nz, ny, nx))] * 3)
        empty = s.device_bytes()
        for role in Z.moment_roles(n):
            x0, y0, z0, where = Z.moments_cloud(shape, n, role, 11)
            s.tracers_set(x0, y0, z0)
            if role == "lost":   # (the first cloud of this context: no sort has made its scratch yet)
                assert s.device_bytes() == empty + 56 * n + (nwg + 1) * 12 * 8, (n, "partials", nwg)
            s.tracers_advance(2.0 ** -10, nsub=Z.MOMENT_NSUB)   # 120 cells along x: every particle wraps at least once
            m = s.tracers_moments()
            x, y, z, wx, wy = s.tracers_get()
            alive = ~np.isnan(x0)
            assert wx[alive].min() >= 1 and wy[alive].max() <= -1 and not wx[~alive].any() and T.same(z[alive], z0[alive])
            assert np.array_equal(np.isnan(x), ~alive)
            want = Z.moments_exact(n, z0)
            assert m.tolist() == want, (n, role, where)   # every term and every partial sum is a small dyadic number: exact in any order
            assert m[0] + m[1] == n and m[1] == sum(k in ("lost", "second batch") for k in where)
            if "z_min" in where:
                assert m[10] == 0.125
            if "z_max" in where:
                assert m[11] == nz - 1 - 0.125
            s.tracers_sort()   # other slots, other partials: the same numbers
            assert s.tracers_moments().tolist() == want, (n, role, "sorted")


def _moment_terms(shape, c):
    """the terms of the eight sums of the alive particles of a cloud {x, y, z, x0, y0, z0, wx, wy}, as the header forms them"""
    alive = ~np.isnan(c["x"])
    dx = (c["x"][alive] - c["x0"][alive]) + c["wx"][alive].astype(np.float64) * float(shape[0])
    dy = (c["y"][alive] - c["y0"][alive]) + c["wy"][alive].astype(np.float64) * float(shape[1])
    dz = c["z"][alive] - c["z0"][alive]
    za = c["z"][alive]
    return alive, [dx, dy, dz, dx * dx, dy * dy, dz * dz, za, za * za]


def test_moments_on_random_displacements_lie_within_the_a_priori_bound_at_33_partials(pkg, inputs):
    n = 131073
    assert Z.levels(n)[0] == 33
    shape = Z.SHAPES["R"]
    u, E = inputs["R"]
    p = _params(pkg, shape)
    x0, y0, z0 = Z.special_cloud(shape, n, 91)
    x, y, z, wx, wy = pkg.tracers_advance_host(p, u, x0, y0, z0, E=E, mu=T.MU, h=T.substep(p), nsub=7)
    alive, terms = _moment_terms(shape, dict(x=x, y=y, z=z, x0=x0, y0=y0, z0=z0, wx=wx, wy=wy))
    exact = [math.fsum(t) for t in terms]
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        s.tracers_set(x0, y0, z0)
        s.tracers_advance(T.substep(p), nsub=7, mu=T.MU)
        for when in ("as set", "sorted"):
            m = s.tracers_moments()
            assert m[0] == alive.sum() and m[1] == n - alive.sum() and m[0] + m[1] == n and m[1] >= np.isnan(x0).sum() > n // 102
            assert m[10] == z[alive].min() and m[11] == z[alive].max()   # min and max are exact
            for k, t in enumerate(terms):
                tol = n * 2.0 ** -53 * np.abs(t).sum()
                d = abs(m[2 + k] - exact[k])
                print(f"n {n} {pkg.TRACER_MOMENTS[2 + k]} {when}: {d:.3e} (tol {tol:.3e})")
                assert d <= tol, (pkg.TRACER_MOMENTS[2 + k], when, d, tol)
            assert np.abs(m[2:5]).max() > 1.0
            s.tracers_sort()
        assert not np.array_equal(s.tracers_ids(), np.arange(n))


# ---- 4. cell counts across workgroups --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(Z.CELL_NS))
def test_cell_counts_equal_bincount_across_workgroups(pkg, n):
    assert Z.cell_workgroups(n) == Z.CELL_NS[n]
    nwg = Z.levels(n)[0]
    shape = Z.SHAPES["W"]
    p = _params(pkg, shape)
    x, y, z = Z.cells_cloud(shape, n, 40 + n)
    gone = int(np.isnan(x).sum())
    assert gone > n // 200
    with pkg.Solver(p) as s:
        empty = s.device_bytes()
        s.tracers_set(x, y, z)
        assert s.device_bytes() == empty + 56 * n + (nwg + 1) * 12 * 8   # n is what the workgroup count follows from
        for cells in Z.CELL_GRIDS:
            counts, lost = s.tracers_cell_counts(cells)
            c = T.cell(shape, cells, x, y, z)
            want = np.bincount(c[c >= 0], minlength=cells[0] * cells[1] * cells[2]).reshape(cells[2], cells[1], cells[0])
            assert counts.dtype == np.int64 and np.array_equal(counts, want), (n, cells)
            assert lost == gone and counts.sum() + lost == n, (n, cells)
        assert s.device_bytes() == empty + 56 * n + (nwg + 1) * 96 + (65536 + 1) * 8   # one counter table for every grid
        s.tracers_sort()   # the same cloud in other slots: the same counts
        for cells in ((63, 13, 10), (64, 16, 8)):
            counts, lost = s.tracers_cell_counts(cells)
            c = T.cell(shape, cells, x, y, z)
            assert np.array_equal(counts.ravel(), np.bincount(c[c >= 0], minlength=counts.size)) and lost == gone, (n, cells, "sorted")


def test_all_particles_of_nine_workgroups_in_one_cell(pkg):
    n = 65537
    assert Z.cell_workgroups(n) == 9
    shape = Z.SHAPES["W"]
    rng = np.random.default_rng(5)
    with pkg.Solver(_params(pkg, shape)) as s:
        s.tracers_set(20.0 + rng.uniform(0, 1, n), 30.0 + rng.uniform(0, 1, n), 6.0 + rng.uniform(0, 1, n))
        for cells in ((70, 66, 12), (64, 16, 8), (63, 13, 10), (7, 6, 4), (1, 1, 1)):   # one counter receives every workgroup's total
            counts, lost = s.tracers_cell_counts(cells)
            assert lost == 0 and counts.max() == n and counts.sum() == n and np.count_nonzero(counts) == 1, cells
            assert counts[(6 * cells[2]) // 12, (30 * cells[1]) // 66, (20 * cells[0]) // 70] == n, cells
        nan = np.full(n, np.nan)
        s.tracers_set(nan, nan, nan)   # and the lost ones' counter
        for cells in ((63, 13, 10), (64, 16, 8)):
            counts, lost = s.tracers_cell_counts(cells)
            assert lost == n and not counts.any(), cells


# ---- 5. tracks: the id search at its edges ---------------------------------------------------------------------------------------

SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)
TRACK_VALUES = ("T", "q", "uz")


def _seeded_start(pkg, s):
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


def _same_rows(got, want):
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(T.bits(got)[~nan], T.bits(want)[~nan])


def _track_run(pkg, s, x, y, z, h, each, arm=None):
    """the sequence of tests/test_tracers_sample_gpu.py::test_track_rows_equal_a_twin; arm() is called where the tracks are armed
    and each(k) where a row is recorded"""
    _seeded_start(pkg, s)
    s.tracers_set(x, y, z)
    s.step(4)
    if arm:
        arm()
    for k in range(5):
        s.step(1)
        if k == 2 or k == 4:
            s.tracers_sort()   # in the middle, and a second one
        s.tracers_advance(h, nsub=2, mu=1e-8 if k % 2 else 0.0)
        each(k)


@pytest.mark.parametrize("ntags", Z.TRACK_NTAGS)
@pytest.mark.parametrize("n", Z.TRACK_NS)
def test_track_rows_equal_a_twin_at_the_edges_of_the_find(pkg, n, ntags):
    shape = Z.SHAPES["R"]
    p = _params(pkg, shape)
    x, y, z = T.special_cloud(shape, n, 100)
    h = 40 * p.dt
    tail = n % 4
    twin, slots = [], []
    with pkg.Solver(p) as b:   # the twin first: its sorts say which ids end in the slots the find reads one by one

        def state(k):
            cx, cy, cz, wx, wy = b.tracers_get(by_id=True)
            v = b.tracers_sample(TRACK_VALUES, by_id=True)
            twin.append(np.stack([cx, cy, cz, wx.astype(np.float64), wy.astype(np.float64), *v], axis=1))
            slots.append(b.tracers_ids())

        _track_run(pkg, b, x, y, z, h, state)
        fields_b = b.fields()
    assert np.array_equal(slots[0], np.arange(n)) and np.array_equal(slots[1], np.arange(n)) and not np.array_equal(slots[2], np.arange(n))
    assert np.array_equal(slots[3], slots[2])   # (the second sort, before row 4, may leave a cloud that has hardly moved where it is)
    must = np.concatenate([slots[k][n - tail:] for k in (2, 4)])
    ids = Z.tag_list(n, ntags, must, ntags)
    assert len(set(ids.tolist())) == ntags and np.isin([0, n - 1, Z.TRACK_LOST, *must], ids).all()
    with pkg.Solver(p) as a:
        _track_run(pkg, a, x, y, z, h, lambda k: a.tracks_record(10 + k, 0.25 * k), arm=lambda: a.tracks_arm(ids=ids, values=TRACK_VALUES, capacity=3))
        assert a.tracks_count() == (5, 2) and np.array_equal(a.tracers_ids(), slots[4])
        steps, times, got = a.tracks_read()
        fields_a = a.fields()
    assert got.shape == (3, ntags, 5 + len(TRACK_VALUES))
    assert steps.tolist() == [12, 13, 14] and times.tolist() == [0.5, 0.75, 1.0]
    for r in range(3):
        assert _same_rows(got[r], twin[2 + r][ids]), (n, ntags, r)
        at = slots[2 + r]   # every held row went through the find; the ids of the scalar tail were tagged
        assert np.isin(at[n - tail:], ids).all()
    lost = int(np.flatnonzero(ids == Z.TRACK_LOST)[0])
    assert np.isnan(got[:, lost, :3]).all() and np.isnan(got[:, lost, 5:]).all() and not np.isnan(got[:, lost, 3:5]).any()
    for name in pkg.FIELDS:   # the tracks left the run alone
        assert np.array_equal(T.bits(fields_a[name]), T.bits(fields_b[name])), name


# ---- 6. sample and advance at 17 runs --------------------------------------------------------------------------------------------

def test_sample_and_advance_equal_the_host_at_65537(pkg):
    n = 65537
    shape = Z.SHAPES["R"]
    p = _params(pkg, shape)
    f = S.all_fields(shape, 977)
    u, E = [f[k] for k in UE[:3]], [f[k] for k in UE[3:]]
    x, y, z = Z.special_cloud(shape, n, 60 + n)
    with pkg.Solver(p) as s:
        s.set_fields(f)
        s.tracers_set(x, y, z)
        want = pkg.tracers_sample_host(p, S.NAMES, f, x, y, z)
        assert len(S.NAMES) == 12 and S.same_sample(s.tracers_sample(S.NAMES), want)
        assert np.isnan(want[:, 40::101]).all() and np.isnan(want).sum() == 12 * np.isnan(x).sum()
        s.tracers_advance(T.substep(p), nsub=7, mu=T.MU)
        got = s.tracers_get()
        host = pkg.tracers_advance_host(p, u, x, y, z, E=E, mu=T.MU, h=T.substep(p), nsub=7)
        for k, name in enumerate(("x", "y", "z")):
            assert T.same(got[k], host[k]), name
        assert np.array_equal(got[3], host[3]) and np.array_equal(got[4], host[4]) and host[3].any() and host[4].any()
        assert np.isnan(host[0]).sum() >= np.isnan(x).sum() > n // 102
        assert S.same_sample(s.tracers_sample(S.NAMES), pkg.tracers_sample_host(p, S.NAMES, f, *host[:3]))
