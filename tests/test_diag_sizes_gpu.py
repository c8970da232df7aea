"""GPU tests of the field diagnostics past every size threshold of their kernels (csrc/stats.hip, monitor.hip, modes.hip, hist.hip,
diag.hip, section.hip, spectrum.hip, snapshot.hip).  The other diagnostics tests stop at planes of 19 200 nodes and contexts of 51
planes, where every two-level kernel runs its first level only: one batch of workgroup partials, one grid-stride round, plane results
that fit LDS, one workgroup along x, a full batch of spectrum planes.  Here the lattice is chosen per kernel so that the second level
runs (tests/_diag_sizes.py holds the table; tests/test_diag_sizes_cpu.py holds the shapes against the constants of the sources and the
references against brute force), and the byte counts of ekpnp_device_bytes show, per shape, the workgroups that were reached.

No test steps the lattice: a context is created, all eleven arrays are set, read back and held against what was set, and the
diagnostic is called.  On DYADIC fields (integers / 1024) every sum is exact in float64 in any order, so the device must return the
exact sum - computed in int64 from the arrays read back - with ==; a lost, repeated or misplaced partial of any size shows.  What has
a host definition (sections: ekpnp_section_sum; histogram counts: ekpnp_hist_bin; value ranges; snapshots) is held bit for bit
against it on arbitrary fields.  The only tolerances are two inherited ones: the a-priori bound of tests/test_modes_gpu.py on a
non-trivial mode, and 4 u of tests/test_spectrum_gpu.py on one plane against numpy's rfft2.

Contexts are shared per shape through a module fixture and never modified: "dyadic" (the unique largest uz at the last node, the
unique largest |rho - rho0| at the first node of workgroup 16; two buffers on A and E, in place on B, C, D - no diagnostic here
depends on the buffer mode, tests/test_observer_pairs_gpu.py holds that), "twin" (in place; the two extremes swapped, and ONE NaN in
c) and "random" (in place).  The first context of a lattice shape takes 0.5 - 1.7 s to create (its transform plans), every further
one 0.01 s: that, and the first use of the device (3.5 s, in the first test), is most of the file's 15.5 s."""
import math
import time

import numpy as np
import pytest

import _diag_sizes as Z

pytestmark = pytest.mark.gpu
VOLUME = ["uz_max", "u_u", "q", "q_q", "uz_T", "rho_dev", "nonfinite"]
PLATES = ["current_top", "current_bottom", "dTdz_bottom", "dTdz_top"]
TWO_BUFFERS = ("A", "E585", "E586")   # the "dyadic" contexts with two population buffers; those of B, C, D hold one (1.7 GB less in all)
SEEDS = {"A": 11, "B": 12, "C": 13, "D": 14, "E585": 15, "E586": 16, "F": 17, "S": 18}


def _params(pkg, shape, in_place=0):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    p.in_place = in_place
    return p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _eq(a, b):
    """== where neither is NaN, and NaN exactly where the other is"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _set_and_read_back(s, f):
    """the setter is not trusted: the arrays read back are the arrays that were set, Ex, Ey, Ez and phi included, bit for bit"""
    s.set_fields(f)
    back = {n: s.get_field(n) for n in f}
    for n, v in f.items():
        assert _same(back[n], v), n
        back[n].setflags(write=False)
    return back


@pytest.fixture(scope="module")
def ctx(pkg):
    """ctx(key, kind) -> (context, the fields read back from it, its device_bytes before any diagnostic); made once per (shape, kind),
    shared by the tests below and left unchanged (a diagnostic's scratch and rings apart)"""
    cache = {}

    def get(key, kind):
        if (key, kind) not in cache:
            shape = Z.SHAPES[key]
            if kind == "dyadic":
                f, in_place = Z.dyadic_fields(shape, SEEDS[key]), 0 if key in TWO_BUFFERS else 1
            elif kind == "twin":
                f, in_place = Z.dyadic_fields(shape, SEEDS[key] + 100, variant=1, nan=Z.nan_node(shape)), 1
            else:
                f, in_place = Z.random_fields(shape, SEEDS[key] + 200), 1
            t0 = time.perf_counter()
            s = pkg.Solver(_params(pkg, shape, in_place))
            t1 = time.perf_counter()
            cache[(key, kind)] = (s, _set_and_read_back(s, f), s.device_bytes())
            print(f"{key} {kind}: created in {t1 - t0:.2f} s, set and read back in {time.perf_counter() - t1:.2f} s, {s.device_bytes() / 2 ** 20:.0f} MiB")
        return cache[(key, kind)]

    yield get
    for s, _, _ in cache.values():
        s.close()


# ---- 1. plane profiles and running statistics --------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["A", "B", "C", "D"])
def test_plane_sums_are_the_exact_sums(pkg, ctx, key):
    shape = Z.SHAPES[key]
    for kind in ("dyadic", "twin"):
        s, f, _ = ctx(key, kind)
        before = s.device_bytes()
        got = s.plane_sums()
        assert s.device_bytes() - before == Z.stats_bytes(shape, shape[2]), (key, kind, Z.chunk_workgroups(shape))
        exact = Z.plane_sums_exact(f)
        assert got.shape == exact.shape == (24, shape[2])
        bad = np.argwhere(~((got == exact) | (np.isnan(got) & np.isnan(exact))))
        assert bad.size == 0, (key, kind, [(pkg.PROFILE_NAMES[q], z, got[q, z], exact[q, z]) for q, z in bad[:6]])
        assert np.isnan(exact).sum() == (6 if kind == "twin" else 0)   # c, c_c, uz_c, q_Ex, q_Ez, q_q of the NaN's plane
        s.stats_reset()
        s.stats_accumulate()
        s.stats_accumulate()
        acc, n = s.stats_get()
        assert n == 2 and _eq(acc, 2.0 * exact), (key, kind)
        s.stats_reset()


# ---- 2. the monitor -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["A", "B", "C", "D", "E585", "E586"])
def test_monitor_sample_is_exact_and_finds_the_planted_extremes(pkg, ctx, key):
    shape = Z.SHAPES[key]
    nx, ny, nz = shape
    for kind in ("dyadic", "twin"):
        s, f, _ = ctx(key, kind)
        before = s.device_bytes()
        row = s.monitor_sample()
        assert s.device_bytes() - before == Z.monitor_bytes(shape, nz), (key, kind, Z.chunk_workgroups(shape))
        exact = Z.monitor_exact(f, s.p)
        print(f"{key} {kind}: " + ", ".join(f"{n} {v!r}" for n, v in zip(pkg.MONITOR_NAMES, row)))
        bad = [(n, g, e) for n, g, e in zip(pkg.MONITOR_NAMES, row, exact) if not (g == e or (np.isnan(g) and np.isnan(e)))]
        assert not bad, (key, kind, bad)
        # the planted extremes and the NaN, as placed
        assert row[4] == Z.PLANT_UZ and row[9] == Z.PLANT_RHO, (key, kind, row[4], row[9])
        want_nan = [0, 1, 6, 7] if nz == 4 else [6, 7]   # the sums that read c at the NaN's node
        assert np.flatnonzero(np.isnan(row)).tolist() == (want_nan if kind == "twin" else []) and row[10] == (1.0 if kind == "twin" else 0.0)
        # the synchronous diagnostics of diag.hip: the same bits
        cur, um = s.current(), s.umax()
        assert _eq(row[0], cur) and (kind == "twin" or _same(row[0], cur)), (key, kind, row[0], cur)
        assert _same(row[4], um), (key, kind, row[4], um)
        assert _eq(s.monitor_sample(), row)
        # through the ring
        s.monitor_arm(None, every=1, capacity=4)
        s.monitor_record(7, 0.5)
        assert s.monitor_count() == (1, 0)
        steps, times, values = s.monitor_read()
        s.monitor_disarm()
        assert steps.tolist() == [7] and times.tolist() == [0.5] and _same(values[0], row), (key, kind, values[0], row)
        if key.startswith("E"):   # the masks choose which kernels run
            vol, pla = s.monitor_sample(VOLUME), s.monitor_sample(PLATES)
            assert _same(vol[4:], row[4:]) and not vol[:4].any() and _same(pla[:4], row[:4]) and not pla[4:].any(), (key, kind)


# ---- 3. mode amplitudes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["A", "B", "C"])
def test_mode_amplitudes_past_one_batch_of_partials(pkg, ctx, key):
    shape = Z.SHAPES[key]
    nx, ny, nz = shape
    modes = Z.modes_of(shape)
    assert (nx % 64 == 0) == (key == "A")   # A: the ROW64 kernel
    s, f, _ = ctx(key, "dyadic")
    before = s.device_bytes()
    ab = s.mode_amplitudes("uz", modes)
    assert s.device_bytes() - before == Z.modes_bytes(shape, nz), (key, Z.chunk_workgroups(shape))
    assert ab.shape == (16, nz, 2)
    exact = Z.to_int(f["uz"]).sum(axis=(1, 2)) / float(Z.Q)
    assert np.array_equal(ab[0, :, 0], exact) and (ab[0, :, 1] == 0.0).all(), (key, ab[0], exact)   # (0, 0): table entries (1, 0)
    st, ft, _ = ctx(key, "twin")
    one = st.mode_amplitudes("uz", [(0, 0)])
    assert np.array_equal(one[0, :, 0], Z.to_int(ft["uz"]).sum(axis=(1, 2)) / float(Z.Q)) and (one[0, :, 1] == 0.0).all(), key
    worst = 0.0
    for j, (m, n) in enumerate(modes[1:], start=1):
        ct, sn = Z.mode_phase(nx, ny, m, n)
        for z in range(nz):
            v = f["uz"][z]
            bound = Z.mode_bound(v)
            for k, w in enumerate((ct, sn)):
                err = abs(ab[j, z, k] - math.fsum((v * w).ravel().tolist()))
                worst = max(worst, err / bound)
                assert err <= bound, (key, (m, n), z, "ab"[k], ab[j, z, k], err, bound)
    print(f"{key}: largest |gpu - fsum| / bound = {worst:.3e}")
    for j, mode in enumerate(modes):   # a mode's (a, b) whatever is projected beside it (the 16-mode and the 1-mode kernel)
        assert _same(s.mode_amplitudes("uz", [mode])[0], ab[j]), (key, mode)
    s.modes_arm("uz", modes, capacity=2)
    s.modes_record(3, 0.25)
    steps, times, rows = s.modes_read()
    s.modes_disarm()
    assert steps.tolist() == [3] and _same(rows[0], Z.energies(ab)), (key, rows[0], Z.energies(ab))


# ---- 4. histograms and value ranges --------------------------------------------------------------------------------------------------

def _hist_equal(got, want):
    return all(g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("key", ["A", "B"])
def test_histogram_of_128_bins_past_one_batch_of_count_tables(pkg, ctx, key):
    """on the dyadic fields: every value lies ON an edge of the 128 bins of -1 .. 1"""
    shape = Z.SHAPES[key]
    nx, ny, nz = shape
    axis = ("uz", 128, -1.0, 1.0)
    s, f, _ = ctx(key, "dyadic")
    before = s.device_bytes()
    counts, nonfinite = s.hist_planes(axis)
    assert s.device_bytes() - before == Z.hist_bytes(shape, nz, [131]), (key, Z.hist_workgroups(shape, 131))
    assert _hist_equal((counts, nonfinite), Z.hist_counts(f, axis)), key
    assert (counts.sum(axis=1) == nx * ny).all() and not nonfinite.any() and counts[:, -1].sum() >= 1   # the planted 2.0 overflows
    st, ft, _ = ctx(key, "twin")
    axis = ("q", 128, -2.0, 2.0)
    counts, nonfinite = st.hist_planes(axis)
    assert _hist_equal((counts, nonfinite), Z.hist_counts(ft, axis)), key
    assert nonfinite.tolist() == [1 if z == Z.nan_node(shape)[0] else 0 for z in range(nz)]   # the NaN is counted apart
    assert (counts.sum(axis=1) + nonfinite == nx * ny).all()


@pytest.mark.parametrize("key", ["C", "D"])
def test_histograms_and_value_range_past_every_chunk_and_batch(pkg, ctx, key):
    shape = Z.SHAPES[key]
    nx, ny, nz = shape
    P = nx * ny
    s, f, _ = ctx(key, "random")
    before = s.device_bytes()
    strides, held = [], {}
    for name, (a, b, _) in Z.HIST_SPECS.items():
        counts, nonfinite = s.hist_planes(a, b)
        strides.append(Z.hist_stride(a, b))
        assert s.device_bytes() - before == Z.hist_bytes(shape, nz, strides), (key, name, Z.hist_workgroups(shape, strides[-1]))
        assert _hist_equal((counts, nonfinite), Z.hist_counts(f, a, b)), (key, name)
        assert (counts.reshape(nz, -1).sum(axis=1) == P).all() and not nonfinite.any(), (key, name)
        assert counts.reshape(nz, -1)[:, 0].sum() > 0 and counts.reshape(nz, -1)[:, -1].sum() > 0, (key, name)   # both outer cells fill
        held[name] = counts
    for name in ("uz", "q"):   # the unique minimum in the last partial, the unique maximum in partial 64 (D) / 16 (C)
        lo, hi = s.value_range(name)
        v = Z.value(f, name).reshape(nz, P)
        assert np.array_equal(lo, np.nanmin(v, axis=1)) and np.array_equal(hi, np.nanmax(v, axis=1)), (key, name, lo, hi)
        assert np.array_equal(lo, v[:, P - 1]) and np.array_equal(hi, v[:, Z.range_top_node(shape)])
    assert s.device_bytes() - before == Z.hist_bytes(shape, nz, strides, ranges=True)
    for name in ("uz128", "q_uz"):   # a ring row over planes 1 .. 2 is the sum of those planes
        a, b, _ = Z.HIST_SPECS[name]
        s.hist_arm(a, b, planes=(1, 2), capacity=2)
        s.hist_record(5, 0.75)
        steps, times, rows, bad = s.hist_read()
        s.hist_disarm()
        assert steps.tolist() == [5] and np.array_equal(rows[0], held[name][1] + held[name][2]) and bad.tolist() == [0], (key, name)
    # a NaN is counted apart: q of the twin, whose dyadic values lie on the edges of 4096 bins of -2 .. 2
    st, ft, _ = ctx(key, "twin")
    axis = ("q", 4096, -2.0, 2.0)
    counts, nonfinite = st.hist_planes(axis)
    assert _hist_equal((counts, nonfinite), Z.hist_counts(ft, axis)), key
    assert nonfinite.tolist() == [1 if z == Z.nan_node(shape)[0] else 0 for z in range(nz)] and (counts.sum(axis=1) + nonfinite == P).all()


# ---- 5. sections -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["C", "D"])
def test_sections_past_one_workgroup_and_two_row_tiles(pkg, ctx, key):
    shape = Z.SHAPES[key]
    nx, ny, nz = shape
    s, f, _ = ctx(key, "random")
    values = {n: Z.value(f, n) for n in pkg.SECTION_VALUES}
    before = s.device_bytes()
    largest = 0
    for across, nkeep in (("x", ny), ("y", nx)):
        for tag, (lo, hi) in Z.section_ranges(shape, across).items():
            got = s.section(None, across, (lo, hi))
            largest = max(largest, 12 * nz * nkeep * 8)
            assert s.device_bytes() - before == largest
            want = np.stack([Z.section_ref(pkg, values[n], across, lo, hi) for n in pkg.SECTION_VALUES])   # every entry: ekpnp_section_sum
            assert got.shape == (12, nz, nkeep) and _same(got, want), (key, across, tag, np.argwhere(_bits(got) != _bits(want))[:5])
            two = s.section(None, across, (lo, hi), [1, 3])
            assert _same(two, want[:, [1, 3]]), (key, across, tag, "planes 1, 3")
            if tag == "cut":   # lo == hi: the field's own bits
                cut = np.stack([v[:, :, lo] if across == "x" else v[:, lo, :] for v in values.values()])
                assert _same(got, cut), (key, across)


# ---- 6. snapshot -------------------------------------------------------------------------------------------------------------------------

def test_snapshot_of_rows_of_six_chunks(pkg, ctx):
    """331 and 397 are prime: cx = cy = 1 is all that divides them.  cz has to divide nz - 1: (1, 1, 1) and (1, 1, 3) on the four
    planes of C; (1, 1, 2) is refused there and runs on the nine planes of S (test_two_uneven_slabs_equal_the_single_context)"""
    s, f, _ = ctx("C", "random")
    with pytest.raises(pkg.EkpnpError) as e:
        s.snapshot(None, (1, 1, 2))
    assert "cz = 2 does not divide nz - 1 = 3" in str(e.value)
    for coarsen in ((1, 1, 1), (1, 1, 3)):
        _snapshot_equals_the_reference(pkg, s.snapshot(None, coarsen), f, coarsen)


def _snapshot_equals_the_reference(pkg, got, f, coarsen):
    assert list(got) == pkg.FIELDS
    for n in pkg.FIELDS:
        want = Z.snapshot_ref(f[n], coarsen)
        assert got[n].dtype == want.dtype == np.float32 and got[n].shape == want.shape == ((f[n].shape[0] - 1) // coarsen[2] + 1, 397, 331)
        assert np.array_equal(got[n].view(np.uint32), want.view(np.uint32)), (n, coarsen, np.argwhere(got[n] != want)[:4])


# ---- 7. spectrum: a batch of fifteen planes and a batch of one ------------------------------------------------------------------------

def test_spectrum_in_batches_of_fifteen_and_one(pkg):
    shape = Z.SHAPES["F"]
    nx, ny, nz = shape
    assert Z.spectrum_batch(shape) == 15 and nz == 16
    f = Z.dyadic_fields(shape, SEEDS["F"], names=["uz"])
    with pkg.Solver(_params(pkg, shape, in_place=1)) as s:
        uz = _set_and_read_back(s, f)["uz"]
        nshell = len(s.spectrum_shells()[1])
        before = s.device_bytes()
        shells, peaks = s.spectrum("uz", list(range(nz)))   # planes 0 .. 14 in the first batch, plane 15 alone in the second
        assert s.device_bytes() - before >= Z.spectrum_buffer_bytes(shape, nz, nshell)   # (the transform's own work area comes on top)
        assert shells.shape == (nz, nshell) and peaks.shape == (nz, 3)
        for z in range(nz):   # "the same bits whatever is transformed beside a plane"
            s1, p1 = s.spectrum("uz", [z])
            assert _same(s1[0], shells[z]) and _same(p1[0], peaks[z]), z
        every, every_peaks = s.spectrum("uz")
        assert _same(every, shells) and _same(every_peaks, peaks)
        for z in (0, 14, 15):   # the last of the first batch, the only one of the second
            P = s.spectrum_plane("uz", z)
            assert tuple(peaks[z]) == Z.spectrum_peak(P), (z, peaks[z])
        err = np.abs(P - Z.rfft2_power(uz[15]))
        tol = Z.power_tolerance(uz[15])
        print(f"F: largest |P - rfft2| / (4 u) = {err.max() / tol:.3e}")
        assert (err <= tol).all(), (err.max(), tol)


# ---- 8. two uneven slabs of C's plane, in place -----------------------------------------------------------------------------------------

def test_two_uneven_slabs_equal_the_single_context(pkg):
    shape = Z.SHAPES["S"]
    nx, ny, nz = shape
    p = _params(pkg, shape, in_place=1)
    f = Z.dyadic_fields(shape, SEEDS["S"])
    r = Z.random_fields(shape, SEEDS["S"] + 200)
    axis, _, _ = Z.HIST_SPECS["q4096"]
    modes = Z.modes_of(shape)[:3]
    with pkg.Solver(p) as s, pkg.Group(p, 2, devices=[0, 0]) as g:
        assert [g.slab_extent(i) for i in range(2)] == [(0, 4), (4, 5)]
        # dyadic fields: the exact sums, which a group returns whatever the order in which its slabs are added
        back = _set_and_read_back(s, f)
        _set_and_read_back(g, f)
        sums = s.plane_sums()
        assert np.array_equal(sums, Z.plane_sums_exact(back)) and _same(g.plane_sums(), sums)
        row, grow = s.monitor_sample(), g.monitor_sample()
        exact = Z.monitor_exact(back, s.p)
        assert np.array_equal(row, exact), (row, exact)
        assert _same(grow, row), (grow, row)
        ab = s.mode_amplitudes("uz", modes)
        assert np.array_equal(ab[0, :, 0], Z.to_int(back["uz"]).sum(axis=(1, 2)) / float(Z.Q)) and _same(g.mode_amplitudes("uz", modes), ab)
        # arbitrary fields: what is reduced per plane or per line has the single context's bits
        back = _set_and_read_back(s, r)
        _set_and_read_back(g, r)
        assert _same(g.plane_sums(), s.plane_sums())
        hs, hg = s.hist_planes(axis), g.hist_planes(axis)
        assert _hist_equal(hg, hs) and _hist_equal(hs, Z.hist_counts(back, axis))
        for across in ("x", "y"):
            lo, hi = Z.section_ranges(shape, across)["odd"]
            got = s.section(["uz", "q"], across, (lo, hi))
            want = np.stack([Z.section_ref(pkg, Z.value(back, n), across, lo, hi) for n in ("uz", "q")])
            assert _same(got, want) and _same(g.section(["uz", "q"], across, (lo, hi)), got), across
        assert _same(g.mode_amplitudes("uz", modes), s.mode_amplitudes("uz", modes))
        snap = s.snapshot(None, (1, 1, 2))     # planes 0, 2, 4, 6, 8 of rows of six x chunks
        _snapshot_equals_the_reference(pkg, snap, back, (1, 1, 2))
        gsnap = g.snapshot(None, (1, 1, 2))    # (slab 1 starts at plane 4: its first sampled plane is its own first)
        assert all(np.array_equal(gsnap[n].view(np.uint32), snap[n].view(np.uint32)) for n in pkg.FIELDS)
