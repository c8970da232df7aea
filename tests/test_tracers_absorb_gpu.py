"""GPU tests of the absorbing plates of the tracers (csrc/tracers.hip: k_tracers_advance_absorbing, k_landings_hist, k_landings_map;
include/ekpnp.h: ekpnp_tracers_advance_absorbing, ekpnp_landings_*; `ekpnp_main --tracers-absorb`).  Every test here fails on the
parent commit: the calls do not exist there.

ekpnp_tracers_advance_absorbing_host is the definition (tests/test_tracers_absorb_cpu.py holds it against a numpy transcription), so
the device is compared with it EXACTLY: all eight arrays of the cloud, read through the cloud's own file, and the six arrays of the
landing record, read through ekpnp_landings_get.  The two reductions are counts: exact as well.  Nothing here has a tolerance.

Lattices: W 70 x 66 x 13, O 35 x 33 x 5, R 40 x 12 x 17 and T 70 x 66 x 17 of the tracer tests; M 128 x 64 x 5, whose plate has the
8192 cells that no longer count in LDS.  n = 1 (one lane), 63 / 64 / 65 (a wavefront and either side), 257 (one past a workgroup),
1000 (a ragged workgroup), 4097; 20 000 for the reductions, whose workgroups take runs of 8192 particles."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _tracers_absorb_ref as A
import _tracers_brownian_ref as B
import _tracers_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
SHAPES = A.SHAPES
NS = (1, 63, 64, 65, 257, 1000, 4097)
NBIG = 20000   # three workgroups of the reductions (runs of 256 x 32 = 8192 particles), the last one ragged
UE = ("ux", "uy", "uz", "Ex", "Ey", "Ez")
ARRAYS = ("x", "y", "z", "x0", "y0", "z0", "wx", "wy")
NOISE = A.NOISE
NAMES = {1: "bottom", 2: "top", 3: "both"}


def _params(pkg, shape, in_place=0):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    p.in_place = in_place
    return p


@pytest.fixture(scope="module")
def inputs(pkg):
    """per lattice: (u, E) random fields and a cloud of NBIG positions - the special ones in front, some on and next to the plates and
    the periodic edges; made once, never modified"""
    out = {}
    for k, s in SHAPES.items():
        u, E = T.random_fields(s, 381 + len(out), T.U_SCALE, T.E_SCALE)
        x, y, z = A.cloud(s, NBIG, 391 + len(out))
        for a in (*u, *E, x, y, z):
            a.setflags(write=False)
        out[k] = (u, E, x, y, z)
    return out


@pytest.fixture(scope="module")
def host(pkg, inputs):
    """host(shape, n, nsub, mu, walls, epoch=0, start=None) -> ekpnp_tracers_advance_absorbing_host of the first n particles (or of an
    earlier result `start`); computed once per case, never modified"""
    cache = {}

    def get(shape, n, nsub, mu, walls=3, epoch=0, start=None):
        key = (shape, n, nsub, mu, walls, epoch, start)
        if key not in cache:
            u, E, x, y, z = inputs[shape]
            p = pkg.default_params(*SHAPES[shape])
            kw = dict(E=E, mu=mu, D=B.diffusivity(p), h=T.substep(p), nsub=nsub, seed=NOISE, epoch=epoch, walls=walls)
            if start is None:
                cache[key] = pkg.tracers_advance_absorbing_host(p, u, x[:n], y[:n], z[:n], **kw)
            else:
                before = cache[start]
                cache[key] = pkg.tracers_advance_absorbing_host(p, u, *before[:5], record=before[5:], **kw)
            for a in cache[key]:
                a.setflags(write=False)
        return cache[key]

    return get


def _put_fields(s, u, E):
    for name, a in zip(UE, (*u, *E)):
        s.set_field(name, a)


def _parse(raw):
    """the cloud's file: ({x, y, z, x0, y0, z0, wx, wy}, ids or None, reserved, reserved2)"""
    assert raw[:8] == b"EKPNPTR1"
    reserved = int(np.frombuffer(raw[20:24], dtype="<i4")[0])
    n = int(np.frombuffer(raw[24:32], dtype="<i8")[0])
    assert len(raw) == 48 + (60 if reserved == 1 else 56) * n, (len(raw), reserved, n)   # the size it always had
    d = np.frombuffer(raw[48:48 + 48 * n], dtype="<f8").reshape(6, n)
    w = np.frombuffer(raw[48 + 48 * n:48 + 56 * n], dtype="<i4").reshape(2, n)
    ids = np.frombuffer(raw[48 + 56 * n:], dtype="<i4") if reserved == 1 else None
    return dict(zip(ARRAYS, [*d, *w])), ids, reserved, int(np.frombuffer(raw[40:48], dtype="<i8")[0])


def _parse_landings(raw):
    """the record's file: ((nx, ny, nz, reserved), n, landed, epoch, the six arrays in the order of ekpnp_landings_get)"""
    assert raw[:8] == b"EKPNPLD1"
    dims = tuple(int(v) for v in np.frombuffer(raw[8:24], dtype="<i4"))
    n, landed, epoch = (int(v) for v in np.frombuffer(raw[24:48], dtype="<i8"))
    assert len(raw) == 48 + 36 * n, (len(raw), n)
    e = np.frombuffer(raw[48:48 + 8 * n], dtype="<i8")
    xy = np.frombuffer(raw[48 + 8 * n:48 + 24 * n], dtype="<f8").reshape(2, n)
    w = np.frombuffer(raw[48 + 24 * n:], dtype="<i4").reshape(3, n)
    return dims, n, landed, epoch, (e, w[0], xy[0], xy[1], w[1], w[2])


def _dump(s, path):
    s.tracers_save(str(path), time=0.5)
    return _parse(open(path, "rb").read())


def _assert_eight(cloud, start, want, what):
    """all eight arrays: the position and the image counts are the host's, the start is the start"""
    for k, name in enumerate(("x", "y", "z")):
        assert T.same(cloud[name], want[k]), (what, name, np.flatnonzero(T.bits(cloud[name]) != T.bits(want[k]))[:5])
        assert T.same(cloud[name + "0"], start[k]), (what, name + "0")
    assert cloud["wx"].dtype == np.int32 and np.array_equal(cloud["wx"], want[3]) and np.array_equal(cloud["wy"], want[4]), what


def _assert_cloud(got, want, what):
    for k, name in enumerate(("x", "y", "z")):
        assert T.same(got[k], want[k]), (what, name, np.flatnonzero(T.bits(got[k]) != T.bits(want[k]))[:5])
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]), what


def _assert_record(got, want, what):
    assert A.same_record(got, want), (what, [np.flatnonzero(np.asarray(g) != np.asarray(w))[:5] for g, w in zip(got, want)])


def _absorb(s, nsub, mu, walls=3, **kw):
    s.tracers_advance(T.substep(s.p), nsub=nsub, mu=mu, D=B.diffusivity(s.p), seed=NOISE, absorb=NAMES[walls], **kw)


# ---- 1. the device equals the definition -----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["W", "O", "R", "T"])
def test_device_absorbing_advance_equals_the_host_definition(pkg, inputs, host, shape, tmp_path):
    u, E, x, y, z = inputs[shape]
    p = _params(pkg, SHAPES[shape])
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        for n in NS:
            for walls in ((3, 1, 2) if n == 4097 else (3,)):
                for nsub in (1, 7):
                    for mu in (0.0, T.MU):
                        s.tracers_set(x[:n], y[:n], z[:n])
                        assert s.tracers_size == n and s.tracers_epoch() == 0
                        _absorb(s, nsub, mu, walls)
                        cloud, ids, reserved, reserved2 = _dump(s, tmp_path / "c.bin")
                        want = host(shape, n, nsub, mu, walls)
                        what = (shape, n, nsub, mu, walls)
                        _assert_eight(cloud, (x[:n], y[:n], z[:n]), want, what)
                        _assert_record(s.landings_get(), want[5:], what)
                        assert ids is None and reserved == 0 and reserved2 == nsub and s.tracers_epoch() == nsub
        # the cases did happen at n = 4097, walls 2, seven substeps with a mobility: landings on the top plate, reflections at the
        # bottom one (nobody is held by it), a particle on the plate at entry, lost ones without a landing, wraps before a landing
        want = host(shape, 4097, 7, T.MU, 2)
        top = float(SHAPES[shape][2] - 1)
        alive = ~np.isnan(want[0])
        assert (want[6] == 2).sum() >= 100 and (want[6] == 1).sum() == 0 and (want[2][alive] > 0.0).all()
        assert want[5][4] == 0 and want[5][18] == 0 and want[5][3] != 0          # on the top plate at entry; on the other plate
        assert np.isnan(want[0][12]) and want[5][12] == -1 and (want[5][~alive] == -1).all()
        assert (want[9] != 0).any() and (want[10] != 0).any()
        assert np.array_equal(want[2][want[5] >= 0], np.full((want[5] >= 0).sum(), top))


def test_in_place_gives_the_same_bits(pkg, inputs, host):
    u, E, x, y, z = inputs["W"]
    with pkg.Solver(_params(pkg, SHAPES["W"], in_place=1)) as s:
        _put_fields(s, u, E)
        for mu in (0.0, T.MU):
            s.tracers_set(x[:1000], y[:1000], z[:1000])
            _absorb(s, 7, mu)
            want = host("W", 1000, 7, mu)
            _assert_cloud(s.tracers_get(), want, ("in place", mu))
            _assert_record(s.landings_get(), want[5:], ("in place", mu))


# ---- 2. interplay ------------------------------------------------------------------------------------------------------

def test_a_sorted_cloud_lands_where_its_unsorted_twin_lands(pkg, inputs, host):
    """the record is keyed by id: this fails if k_tracers_advance_absorbing indexes it by slot, or draws by slot"""
    u, E, x, y, z = inputs["T"]
    p = _params(pkg, SHAPES["T"])
    n = 4097
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        for s in (a, b):
            _put_fields(s, u, E)
            s.tracers_set(x[:n], y[:n], z[:n])
        a.tracers_sort()
        ids = a.tracers_ids()
        assert (ids != np.arange(n)).sum() > n // 2   # the sort did move the particles
        for s in (a, b):
            _absorb(s, 3, T.MU)
        _assert_cloud(a.tracers_get(by_id=True), b.tracers_get(), "sorted, then advanced")
        _assert_record(a.landings_get(), b.landings_get(), "sorted, then advanced")
        a.tracers_sort()                              # the stuck ones share the keys of the plate planes; the record is not touched
        assert not np.array_equal(a.tracers_ids(), ids)
        _assert_record(a.landings_get(), b.landings_get(), "sorted again")
        for s in (a, b):
            _absorb(s, 4, T.MU)
        first = ("T", n, 3, T.MU, 3, 0, None)
        host(*first[:5])
        want = host("T", n, 4, T.MU, 3, 3, first)
        _assert_cloud(a.tracers_get(by_id=True), want, "sorted twice")
        _assert_cloud(b.tracers_get(), want, "the twin")
        _assert_record(a.landings_get(), want[5:], "sorted twice")
        _assert_record(b.landings_get(), want[5:], "the twin")
        slot = a.landings_get(by_id=False)            # in slot order: the order of tracers_get()
        ga = a.tracers_get()
        held = slot[0] >= 0
        assert held.sum() > 500 and T.same(slot[2][held], ga[0][held]) and np.array_equal(slot[4][held], ga[3][held])
        _assert_cloud(want, host("T", n, 7, T.MU), "two calls equal one")
        _assert_record(want[5:], host("T", n, 7, T.MU)[5:], "two calls equal one")
        assert a.tracers_epoch() == 7 and b.tracers_epoch() == 7
        # the diagnostics take a stuck particle for an alive one
        m = b.tracers_moments()
        assert m[0] == (~np.isnan(want[0])).sum() and m[1] == np.isnan(want[0]).sum() and m[10] == 0.0 and m[11] == float(SHAPES["T"][2] - 1)
        counts, lost = b.tracers_cell_counts((1, 1, 16))
        assert counts.sum() + lost == n and counts[0, 0, 0] >= (want[6] == 1).sum() and counts[15, 0, 0] >= (want[6] == 2).sum()
        # a Brownian advance moves the stuck ones again and the record keeps the first landing
        before = b.landings_get()
        b.tracers_advance(T.substep(p), nsub=1, mu=T.MU, D=B.diffusivity(p), seed=NOISE)
        zb = b.tracers_get()[2]
        assert ((zb > 0.0) & (zb < 16.0))[~np.isnan(zb)].all()
        _assert_record(b.landings_get(), before, "after a Brownian advance")


def test_save_both_files_load_both_and_continue_is_not_having_stopped(pkg, inputs, host, tmp_path):
    u, E, x, y, z = inputs["W"]
    p = _params(pkg, SHAPES["W"])
    cpath, lpath = str(tmp_path / "cloud.bin"), str(tmp_path / "landings.bin")
    n = 1000
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        _put_fields(a, u, E)
        _put_fields(b, u, E)
        a.tracers_set(x[:n], y[:n], z[:n])
        _absorb(a, 3, T.MU)
        a.tracers_save(cpath, time=0.125)
        a.landings_save(lpath)
        raw, lraw = open(cpath, "rb").read(), open(lpath, "rb").read()
        cloud, ids, reserved, reserved2 = _parse(raw)
        assert len(raw) == 48 + 56 * n and ids is None and reserved == 0 and reserved2 == 3   # EKPNPTR1 has the size it always had
        dims, m, landed, epoch, rec = _parse_landings(lraw)
        first = host("W", n, 3, T.MU)
        assert dims == (70, 66, 13, 0) and m == n and epoch == 3 and landed == (first[6] != 0).sum() > 50
        _assert_record(rec, first[5:], "the file")
        assert b.tracers_load(cpath) == 0.125 and b.tracers_epoch() == 3
        with pytest.raises(pkg.EkpnpError) as e:
            b.landings_get()
        assert "tracers: no landing record" in str(e.value)
        b.landings_load(lpath)
        _assert_record(b.landings_get(), first[5:], "loaded")
        for s in (a, b):
            _absorb(s, 4, T.MU)
        want = host("W", n, 7, T.MU)
        for s in (a, b):
            _assert_cloud(s.tracers_get(), want, "continued")
            _assert_record(s.landings_get(), want[5:], "continued")
        # a sorted cloud: the ids travel in the cloud's file, the record is by id and needs none
        a.tracers_sort()
        a.tracers_save(cpath, time=0.5)
        a.landings_save(lpath)
        assert os.path.getsize(cpath) == 48 + 60 * n and os.path.getsize(lpath) == 48 + 36 * n
        b.tracers_load(cpath)
        b.landings_load(lpath)
        for s in (a, b):
            _absorb(s, 2, 0.0)
        _assert_cloud(b.tracers_get(), a.tracers_get(), "sorted and continued")
        _assert_record(b.landings_get(), a.landings_get(), "sorted and continued")
        whole = ("W", n, 7, T.MU, 3, 0, None)
        _assert_record(a.landings_get(), host("W", n, 2, 0.0, 3, 7, whole)[5:], "sorted, by id")
        _assert_cloud(a.tracers_get(by_id=True), host("W", n, 2, 0.0, 3, 7, whole), "sorted, by id")

        # every refusal of the record's file, with its number; the record in memory is left alone
        before = b.landings_get()

        def refused(name, edit, msg, s=b):
            bad = bytearray(lraw)
            edit(bad)
            path = str(tmp_path / (name + ".bin"))
            open(path, "wb").write(bytes(bad))
            with pytest.raises(pkg.EkpnpError) as e:
                s.landings_load(path)
            assert msg in str(e.value) and "status 1" in str(e.value), (name, str(e.value))

        def put(at, dtype, v):
            def edit(bad):
                bad[at:at + np.dtype(dtype).itemsize] = np.array([v], dtype).tobytes()
            return edit

        def cut(bad):
            del bad[-4:]

        landed_id = int(np.flatnonzero(first[5] >= 0)[0])
        free_id = int(np.flatnonzero(first[5] < 0)[0])
        wall_at = lambda i: 48 + 24 * n + 4 * i
        refused("magic", put(0, "<i8", 7), "not a landing file (EKPNPLD1)")
        refused("lattice", put(8, "<i4", 71), "lattice 71 x 66 x 13, not of 70 x 66 x 13")
        refused("count", put(24, "<i8", n + 1), "n = %d in the landing file, the cloud has %d" % (n + 1, n))
        refused("short", cut, "shorter than its %d entries" % n)
        refused("reserved", put(20, "<i4", 2), "reserved = 2")
        refused("wall", put(wall_at(free_id + 1), "<i4", 3), "id %d: wall = 3" % (free_id + 1))
        refused("pair1", put(wall_at(free_id), "<i4", 1), "id %d: epoch = -1 with wall = 1" % free_id)
        refused("pair2", put(wall_at(landed_id), "<i4", 0), "id %d: epoch = %d with wall = 0" % (landed_id, first[5][landed_id]))
        refused("pair3", put(48 + 8 * free_id, "<i8", -2), "id %d: epoch = -2" % free_id)
        refused("late", put(48 + 8 * landed_id, "<i8", 4), "id %d: epoch = 4 above the file's epoch 3" % landed_id)
        refused("landed", put(32, "<i8", landed + 1), "landed = %d in the landing file, which holds %d" % (landed + 1, landed))
        _assert_record(b.landings_get(), before, "refused loads")
        b.tracers_set(x[:10], y[:10], z[:10])
        refused("other cloud", lambda bad: None, "n = %d in the landing file, the cloud has 10" % n)
        b.tracers_release()
        refused("no cloud", lambda bad: None, "no cloud")


# ---- 3. the reductions -------------------------------------------------------------------------------------------------

HISTS = ((3, 0, 1, 1), (3, 0, 1, 64), (3, 0, 1, 4096), (1, 0, 1, 64), (2, 0, 1, 64), (3, 2, 3, 2), (1, 3, 1000, 64), (2, 5, 1, 4096), (3, 8, 1, 1))   # walls, e0, width, nbins


def _check_reductions(s, dims, rec, n, maps, what):
    for walls, e0, width, nbins in HISTS:
        counts, none = s.landings_hist(e0=e0, width=width, nbins=nbins, absorb=NAMES[walls])
        wc, wn = A.hist(rec, walls, e0, width, nbins)
        assert counts.dtype == np.int64 and counts.shape == (nbins + 2,) and np.array_equal(counts, wc) and none == wn and counts.sum() + none == n, (what, walls, e0, width, nbins)
    for wall in (1, 2):
        for bx, by in maps:
            for e_lo, e_hi in ((0, 2 ** 63 - 1), (2, 4), (0, 0), (5, 5), (9, 3)):
                counts, other = s.landings_map(wall, (bx, by), e_lo, e_hi)
                wc, wo = A.deposit(dims, rec, wall, bx, by, e_lo, e_hi)
                assert counts.shape == (by, bx) and np.array_equal(counts, wc) and other == wo and counts.sum() + other == n, (what, wall, bx, by, e_lo, e_hi)


def test_histogram_and_map_equal_numpy_on_the_host_records(pkg, inputs, host):
    u, E, x, y, z = inputs["W"]
    dims = SHAPES["W"]
    p = _params(pkg, dims)
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        for n in (1, 64, 257, 4097, NBIG):
            # a spread record: seven substeps from the shared cloud; its epochs are 0 (on the plate at entry) .. 7
            s.tracers_set(x[:n], y[:n], z[:n])
            _absorb(s, 7, T.MU)
            rec = host("W", n, 7, T.MU)[5:]
            if n >= 4097:
                assert len(set(rec[0])) == 9 and (rec[1] == 1).sum() > 100 and (rec[1] == 2).sum() > 100 and (rec[1] == 0).sum() > 100
            _check_reductions(s, dims, rec, n, ((1, 1), (8, 8), (70, 66), (3, 1), (1, 5)), ("spread", n))
            # nobody has landed: every count is in `none` / `elsewhere`
            s.landings_reset()
            _check_reductions(s, dims, A.empty_record(n), n, ((1, 1), (8, 8)), ("empty", n))
            counts, none = s.landings_hist(nbins=4)
            assert none == n and not counts.any()
            # every landing in ONE cell, every lane of a wavefront at one counter: a cloud set on the plate
            s.tracers_set(np.full(n, 33.25), np.full(n, 20.5), np.full(n, 12.0))
            for k in range(2):
                s.tracers_advance(T.substep(p), nsub=2, D=B.diffusivity(p), seed=1, absorb="top")
            one = pkg.tracers_advance_absorbing_host(p, u, np.full(n, 33.25), np.full(n, 20.5), np.full(n, 12.0), D=B.diffusivity(p), h=T.substep(p), nsub=2, seed=1, walls=2)
            assert (one[5] == 0).all() and (one[6] == 2).all()
            _assert_record(s.landings_get(), one[5:], ("one cell", n))
            assert s.tracers_epoch() == 4
            _check_reductions(s, dims, one[5:], n, ((1, 1), (8, 8), (70, 66)), ("one cell", n))
            counts, other = s.landings_map("top", (8, 8))
            assert counts[2, 3] == n and other == 0 and s.landings_map("bottom", (8, 8))[1] == n
            counts, none = s.landings_hist(e0=0, width=1, nbins=64, absorb="top")
            assert counts[1] == n and none == 0


def test_maps_on_either_side_of_the_lds_table(pkg):
    """M 128 x 64 x 5: 127 x 64 = 8128 cells is the largest map of this plate whose 8129 counters fit the 8192 of the workgroup's LDS
    (8191 is prime and 8190 has no factors within 128 x 64), 128 x 64 = 8192 the smallest that does not"""
    dims = (128, 64, 5)
    p = _params(pkg, dims)
    n = NBIG
    rng = np.random.default_rng(77)
    x, y, z = rng.uniform(0, 128, n), rng.uniform(0, 64, n), rng.uniform(0.25, 3.75, n)
    zero = np.zeros((5, 64, 128))
    h = 1.0
    D = (1.5 * p.dz) ** 2 / (6.0 * h)   # kicks of up to a cell and a half
    with pkg.Solver(p) as s:
        for name in UE[:3]:
            s.set_field(name, zero)
        s.tracers_set(x, y, z)
        s.tracers_advance(h, nsub=6, D=D, seed=NOISE, absorb="both")
        rec = pkg.tracers_advance_absorbing_host(p, [zero, zero, zero], x, y, z, D=D, h=h, nsub=6, seed=NOISE, walls=3)[5:]
        _assert_record(s.landings_get(), rec, "M")
        assert (rec[1] == 1).sum() > 2000 and (rec[1] == 2).sum() > 2000
        for wall in (1, 2):
            for bx, by in ((127, 64), (128, 64), (128, 63), (90, 91 - 27)):
                for e_lo, e_hi in ((0, 2 ** 63 - 1), (2, 4)):
                    counts, other = s.landings_map(wall, (bx, by), e_lo, e_hi)
                    wc, wo = A.deposit(dims, rec, wall, bx, by, e_lo, e_hi)
                    assert np.array_equal(counts, wc) and other == wo and counts.sum() + other == n, (wall, bx, by, e_lo)
        assert s.landings_map(1, (128, 64))[0].max() >= 2   # two landings in a cell of the global table
        for kw, number in ((dict(wall=0, cells=(8, 8)), "wall = 0"), (dict(wall=3, cells=(8, 8)), "wall = 3"), (dict(wall=1, cells=(129, 8)), "bx = 129"),
                           (dict(wall=1, cells=(8, 65)), "by = 65"), (dict(wall=2, cells=(128, 64 * 9)), "by = 576")):
            with pytest.raises(pkg.EkpnpError) as e:
                s.landings_map(**kw)
            assert number in str(e.value) and "status 1" in str(e.value), kw
        for kw, number in ((dict(e0=-1), "e0 = -1"), (dict(width=0), "width = 0"), (dict(nbins=0), "nbins = 0"), (dict(nbins=4097), "nbins = 4097"), (dict(absorb=0), "walls = 0"),
                           (dict(absorb=4), "walls = 4")):
            with pytest.raises(pkg.EkpnpError) as e:
                s.landings_hist(**kw)
            assert number in str(e.value) and "status 1" in str(e.value), kw


# ---- 4. the record's life ----------------------------------------------------------------------------------------------

SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)


def _seeded_start(pkg, s):
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


def test_the_record_is_made_dropped_cleared_and_freed(pkg, tmp_path):
    p = _params(pkg, SHAPES["R"])
    n = 1000
    no_record = "tracers: no landing record"
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        _seeded_start(pkg, a)
        _seeded_start(pkg, b)
        a.step(5)
        b.step(5)
        state = a.graph_state()
        before = a.device_bytes()
        a.tracers_seed(n=n, seed=1)
        with_cloud = a.device_bytes()
        D = (1.5 * p.dx) ** 2 / (6.0 * p.dt)

        def absent():
            with pytest.raises(pkg.EkpnpError) as e:
                a.landings_get()
            assert no_record in str(e.value) and "status 1" in str(e.value)
            assert a.device_bytes() == with_cloud

        absent()
        a.landings_reset()                                   # nothing to clear, nothing is allocated
        absent()
        for call in (lambda: a.landings_hist(nbins=4), lambda: a.landings_map(1, (2, 2)), lambda: a.landings_save(str(tmp_path / "none.bin"))):
            with pytest.raises(pkg.EkpnpError) as e:
                call()
            assert no_record in str(e.value)
        # Brownian and plain advances make no record
        a.tracers_advance(p.dt, nsub=2, D=D, seed=1)
        a.tracers_advance(p.dt, nsub=2)
        absent()
        for k in range(4):
            a.step(1)
            a.tracers_advance(p.dt, nsub=2, mu=1e-8 if k % 2 else 0.0, D=D, seed=k, absorb="both")
            assert a.device_bytes() == with_cloud + 36 * n   # the record, made by the first absorbing advance, and nothing else
        landed = (a.landings_get()[1] != 0).sum()
        assert landed > 20 and a.tracers_epoch() == 10
        a.landings_hist(nbins=4)
        with_table = a.device_bytes()
        assert with_table == with_cloud + 36 * n + 8 * (pkg.TRACERS_MAX_CELLS + 1)   # the table of the cell counts, shared
        a.landings_map(1, (2, 2))
        a.tracers_cell_counts((2, 2, 2))
        assert a.device_bytes() == with_table
        # reset clears, the next advance records anew (the stuck ones at once, with the call's epoch)
        a.landings_reset()
        rec = a.landings_get()
        assert (rec[0] == -1).all() and (rec[1] == 0).all() and np.isnan(rec[2]).all() and np.isnan(rec[3]).all() and not rec[4].any() and not rec[5].any()
        a.tracers_advance(p.dt, nsub=1, D=D, seed=9, absorb="both")
        rec = a.landings_get()
        assert (rec[1] != 0).sum() >= landed and (rec[0][rec[1] != 0] >= 10).all() and (rec[0] == 10).sum() >= landed
        # seed, set and load drop it: a new cloud has no landings
        a.tracers_save(str(tmp_path / "c.bin"))
        x, y, z = a.tracers_get()[:3]
        for renew in (lambda: a.tracers_seed(n=n, seed=2), lambda: a.tracers_set(x, y, z), lambda: a.tracers_load(str(tmp_path / "c.bin"))):
            a.tracers_advance(p.dt, nsub=1, D=D, seed=9, absorb="top")
            assert a.device_bytes() == with_table
            renew()
            assert a.device_bytes() == with_table - 36 * n
            with pytest.raises(pkg.EkpnpError) as e:
                a.landings_get()
            assert no_record in str(e.value)
        a.tracers_advance(p.dt, nsub=1, D=D, seed=9, absorb="bottom")
        a.tracers_seed(n=2 * n, seed=2)                      # another size: dropped with the cloud it belonged to
        with pytest.raises(pkg.EkpnpError) as e:
            a.landings_get()
        assert no_record in str(e.value)
        a.tracers_advance(p.dt, nsub=1, D=D, seed=9, absorb="bottom")
        assert a.landings_get()[0].size == 2 * n
        # the run was left alone, and release gives everything back
        b.step(4)
        assert a.graph_state() == state and b.graph_state() == state
        fa, fb = a.fields(), b.fields()
        for name in pkg.FIELDS:
            assert np.array_equal(T.bits(fa[name]), T.bits(fb[name])), name
        assert b.device_bytes() == before
        a.tracers_release()
        assert a.device_bytes() == before


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as G
pkg = G.load_package()
p = pkg.default_params(40, 12, 17)
with pkg.Solver(p) as s:
    before = s.device_bytes()
    s.tracers_seed(n=5000, seed=1)
    s.tracers_advance(1e-9, nsub=2)
    cloud = s.device_bytes() - before
    s.tracers_advance(1e-9, nsub=2, mu=1e-8)   # (the E arrays of a lazy solve are not the cloud's)
    before = s.device_bytes()
    s.tracers_advance(1e-9, nsub=2, D=1e-9)
    s.tracers_sort(); s.tracers_moments(); s.tracers_cell_counts((4, 3, 2)); s.tracers_sample(["ux"]); s.tracers_save(sys.argv[1])
    print("PLAIN OK", s.tracers_epoch(), cloud, s.device_bytes() - before)
    try:
        s.tracers_advance(1e-9, nsub=2, D=1e-9, absorb="both")
        print("ABSORBING OK")
    except pkg.EkpnpError as e:
        print("ERR", e)
''' % ROOT


def test_a_context_that_never_absorbs_launches_no_absorbing_kernel_and_allocates_nothing(tmp_path):
    """the library's launch-failure knob (read once per process, hence a child) fails the named kernel's first launch: everything a
    cloud did before this change goes through with the bytes it had - the cloud 56 n + its partials, the sort's scratch 16 n + tables,
    the ids 4 n, the cell table, the sample scratch 8 n - and the absorbing advance reports that kernel by name"""
    env = dict(os.environ, EKPNP_INJECT_LAUNCH_FAILURE="k_tracers_advance_absorbing")
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "c.bin")], env=env, capture_output=True, text=True, timeout=300)
    n = 5000
    cloud, rest = 56 * n + 3 * 12 * 8, (16 * n + 4 * (256 * 2 + 1)) + 4 * n + 8 * 65537 + 8 * n
    assert r.returncode == 0 and "PLAIN OK 2 %d %d" % (cloud, rest) in r.stdout and "ERR" in r.stdout and "kernel k_tracers_advance_absorbing:" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert os.path.getsize(tmp_path / "c.bin") == 48 + 60 * n


# ---- 5. refusals -------------------------------------------------------------------------------------------------------

def test_refusals_of_the_context_calls(pkg, tmp_path):
    p = _params(pkg, SHAPES["W"])
    msg = "tracers: slab contexts are not supported"
    for rank, nranks in ((0, 1), (1, 3)):
        with pkg.Solver(p, rank=rank, nranks=nranks, slab=True) as s:
            calls = (lambda: s.tracers_advance(1e-9, D=1e-9, absorb="both"), lambda: s.landings_get(), lambda: s.landings_reset(), lambda: s.landings_hist(nbins=4),
                     lambda: s.landings_map(1, (2, 2)), lambda: s.landings_save(str(tmp_path / "x.bin")), lambda: s.landings_load(str(tmp_path / "x.bin")))
            for k, call in enumerate(calls):
                with pytest.raises(pkg.EkpnpError) as e:
                    call()
                assert "status 1" in str(e.value) and msg in str(e.value), k
    assert not [m for m in dir(pkg.Group) if "tracers" in m or "landings" in m]   # and a group has no spelling of them
    with pkg.Solver(p) as s:
        for call in (lambda: s.tracers_advance(1e-9, D=1e-9, absorb="both"), lambda: s.landings_reset(), lambda: s.landings_hist(nbins=4), lambda: s.landings_map(1, (2, 2)),
                     lambda: s.landings_save(str(tmp_path / "x.bin"))):
            with pytest.raises(pkg.EkpnpError) as e:
                call()
            assert "no cloud" in str(e.value)
        s.tracers_seed(n=100, seed=1)
        before = s.tracers_get()
        bytes_before = s.device_bytes()
        for kw, number in ((dict(h=1e-9, D=1e-9, absorb=0), "walls = 0"), (dict(h=1e-9, D=1e-9, absorb=4), "walls = 4"), (dict(h=1e-9, D=-1.5, absorb="both"), "D = -1.5"),
                           (dict(h=1e-9, D=float("nan"), absorb="top"), "D = nan"), (dict(h=-0.25, D=0.5, absorb="both"), "D*h = -0.125"),
                           (dict(h=1e-9, D=1e-9, nsub=0, absorb="both"), "nsub = 0"), (dict(h=1e-9, D=1e-9, nsub=4097, absorb="both"), "nsub = 4097"),
                           (dict(h=float("inf"), absorb="both"), "h = inf"), (dict(h=1e-9, mu=float("inf"), absorb="bottom"), "mu = inf")):
            with pytest.raises(pkg.EkpnpError) as e:
                s.tracers_advance(**kw)
            assert number in str(e.value) and "status 1" in str(e.value), kw
        with pytest.raises(ValueError):
            s.tracers_advance(1e-9, absorb="sides")
        assert s.tracers_epoch() == 0 and s.device_bytes() == bytes_before   # a refused call takes no epoch, moves nobody and makes no record
        _assert_cloud(s.tracers_get(), before, "refused")
        with pytest.raises(pkg.EkpnpError) as e:
            s.landings_get()
        assert "tracers: no landing record" in str(e.value)
        s.tracers_advance(1e-9, absorb="both")               # D=None with absorb: 0.0 - drift alone
        assert s.tracers_epoch() == 1 and s.landings_get()[0].size == 100


# ---- 6. the driver -----------------------------------------------------------------------------------------------------

def _run_driver(args, out, code=0):
    out.mkdir()
    env = dict(os.environ, EKPNP_PLACEMENT_TRIES="1")  # the child shares device 0 with this process
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == code, (args, r.stderr[-2000:])
    return out, r.stderr


GEO = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "6", "--seed-pattern", "squares", "--seed-modes", "1,1"]


def test_driver_writes_the_landing_files_of_the_library_calls_in_both_loops(pkg, tmp_path):
    assert os.path.exists(EXE), "ekpnp_main not built"
    p = pkg.default_params(40, 12, 17)
    mu = 1e-9
    D = (1.5 * p.dx) ** 2 / (12.0 * p.dt)   # a kick of up to a cell and a half per substep of 2 dt
    spec = pkg.tracers_spec(n=1000, box=((0, 40), (0, 12), (1, 15)), seed=9)
    with pkg.Solver(p) as s:  # the driver's loop, call by call
        s.initialization()
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-3, noise=0.0, relative=True, seed=1))
        s.fast_Poisson()
        s.init_equilibrium()
        s.tracers_seed(spec)
        t = 0.0
        for i in range(6):
            s.stream_collide_save(t)
            s.fast_Poisson()
            t = t + p.dt
            if (i + 1) % 2 == 0:
                s.tracers_advance(2.0 * p.dt, nsub=3, mu=mu, D=D, seed=77, absorb="both")
        s.landings_save(str(tmp_path / "lib_landings.bin"))
        rec = s.landings_get()
        hist = [s.landings_hist(e0=0, width=2, nbins=5, absorb=w) for w in ("bottom", "top")]
        maps = [s.landings_map(w, (4, 3), 0, 9) for w in (1, 2)]
        assert s.tracers_epoch() == 9
    assert (rec[1] == 1).sum() > 20 and (rec[1] == 2).sum() > 20
    flags = ["--tracers", "1000", "--tracers-seed", "9", "--tracers-every", "2", "--tracers-substeps", "3", "--tracers-mobility", "1e-9",
             "--tracers-diffusivity", repr(D), "--tracers-noise-seed", "77", "--tracers-absorb", "both", "--arrivals-bins", "5", "--deposit-cells", "4,3"]
    loop, _ = _run_driver([*GEO, *flags], tmp_path / "loop")
    batch, _ = _run_driver([*GEO, *flags, "--batch", "1"], tmp_path / "batch")
    for f in ("landings.bin", "arrivals.dat", "deposit.dat", "tracers.dat", "tracers_final.bin"):
        v = (loop / f).read_bytes()
        assert len(v) > 0 and v == (batch / f).read_bytes(), f
    assert (loop / "landings.bin").read_bytes() == (tmp_path / "lib_landings.bin").read_bytes()
    dims, n, landed, epoch, got = _parse_landings((loop / "landings.bin").read_bytes())
    assert dims == (40, 12, 17, 0) and n == 1000 and epoch == 9 and landed == (rec[1] != 0).sum()
    _assert_record(got, rec, "landings.bin")
    lines = (loop / "arrivals.dat").read_text().splitlines()
    assert lines[0].startswith("# ekpnp arrivals nx 40 ny 12 nz 17 n 1000 epoch 9 e0 0 width 2 nbins 5") and len(lines) == 3
    for k, (counts, none) in enumerate(hist):
        assert [int(v) for v in lines[1 + k].split(" ")] == [k + 1, none, *counts]
    lines = (loop / "deposit.dat").read_text().splitlines()
    assert lines[0].startswith("# ekpnp deposit nx 40 ny 12 nz 17 bx 4 by 3 n 1000 epoch 9") and len(lines) == 1 + 2 * 4
    for k, (counts, other) in enumerate(maps):
        assert [int(v) for v in lines[1 + 4 * k].split(" ")] == [k + 1, other]
        assert np.array_equal(np.array([[int(v) for v in ln.split(" ")] for ln in lines[2 + 4 * k:5 + 4 * k]]), counts)
    # the defaults, drift alone (no diffusivity), and the refusals of the flags
    plain, _ = _run_driver([*GEO, "--tracers", "100", "--tracers-absorb", "top"], tmp_path / "plain")
    assert _parse_landings((plain / "landings.bin").read_bytes())[1:4] == (100, 0, 6)
    assert (plain / "arrivals.dat").read_text().splitlines()[0].split(" nbins ")[1].startswith("16") and " bx 8 by 8 " in (plain / "deposit.dat").read_text().splitlines()[0]
    for bad, number in ((["--tracers-absorb", "both"], "there is no cloud to deposit"), (["--tracers", "10", "--tracers-absorb", "sides"], "got sides"),
                        (["--tracers", "10", "--arrivals-bins", "4"], "no plate absorbs"), (["--tracers", "10", "--tracers-absorb", "top", "--arrivals-bins", "5000"], "got 5000"),
                        (["--tracers", "10", "--tracers-absorb", "top", "--deposit-cells", "41,3"], "bx = 41"), (["--tracers", "10", "--tracers-absorb", "top", "--deposit-cells", "4"], "got 4")):
        _, err = _run_driver([*GEO, *bad], tmp_path / ("bad" + "_".join(bad).replace("-", "").replace(",", "_")), code=2)
        assert number in err, err
