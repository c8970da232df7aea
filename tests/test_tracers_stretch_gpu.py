"""GPU tests of the flow-map gradient of the tracers (csrc/tracers.hip: k_tracers_advance_tangent, k_stretch_begin, k_stretch_levels;
include/ekpnp.h: ekpnp_tracers_advance_tangent, ekpnp_tracers_stretch_*; `ekpnp_main --tracers-stretch`).  Every test here fails on
the parent commit: the calls do not exist there.

ekpnp_tracers_advance_tangent_host is the definition (tests/test_tracers_stretch_cpu.py holds it against a numpy transcription), so
the device is compared with it EXACTLY: F on its bit pattern, e, and all eight arrays of the cloud, read through the cloud's own
file.  The histogram of levels is a count: exact as well.  Nothing here has a tolerance.

Lattices: W 70 x 66 x 13, O 35 x 33 x 5, R 40 x 12 x 17 and T 70 x 66 x 17 of the tracer tests.  n = 1 (one lane), 63 / 64 / 65 (a
wavefront and either side), 257 (one past a workgroup), 1000 (a ragged workgroup), 4097 (one past the sort's run of 4096); 20 000
for the histogram, whose workgroups take runs of 8192 particles."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _tracers_ref as T
import _tracers_stretch_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
SHAPES = S.SHAPES
NS = (1, 63, 64, 65, 257, 1000, 4097)
NSUBS = (1, 7, 100)
NBIG = 20000
UE = ("ux", "uy", "uz", "Ex", "Ey", "Ez")
ARRAYS = ("x", "y", "z", "x0", "y0", "z0", "wx", "wy")
NO_RECORD = "tracers: no stretch record"


def _params(pkg, shape, in_place=0):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    p.in_place = in_place
    return p


@pytest.fixture(scope="module")
def inputs(pkg):
    """per lattice: (u, E) random fields and the special cloud of NBIG positions (one lost from the start); made once, never modified"""
    out = {}
    for k, s in SHAPES.items():
        u, E = T.random_fields(s, 671 + len(out), T.U_SCALE, T.E_SCALE)
        x, y, z = T.special_cloud(s, NBIG, 681 + len(out))
        for a in (*u, *E, x, y, z):
            a.setflags(write=False)
        out[k] = (u, E, x, y, z)
    return out


@pytest.fixture(scope="module")
def host(pkg, inputs):
    """host(shape, n, nsub, mu, start=None) -> ekpnp_tracers_advance_tangent_host of the first n particles from a record just begun (or
    from an earlier result, its key given as `start`); computed once per case, never modified"""
    cache = {}

    def get(shape, n, nsub, mu, start=None):
        key = (shape, n, nsub, mu, start)
        if key not in cache:
            u, E, x, y, z = inputs[shape]
            p = pkg.default_params(*SHAPES[shape])
            kw = dict(E=E, mu=mu, h=T.substep(p), nsub=nsub)
            if start is None:
                cache[key] = pkg.tracers_advance_tangent_host(p, u, x[:n], y[:n], z[:n], **kw)
            else:
                b = cache[start]
                cache[key] = pkg.tracers_advance_tangent_host(p, u, b[0], b[1], b[2], F=b[5], e=b[6], wx=b[3], wy=b[4], **kw)
            for a in cache[key]:
                a.setflags(write=False)
        return cache[key]

    return get


def _put_fields(s, u, E):
    for name, a in zip(UE, (*u, *E)):
        s.set_field(name, a)


def _parse(raw):
    """the cloud's file: {x, y, z, x0, y0, z0, wx, wy}"""
    assert raw[:8] == b"EKPNPTR1"
    n = int(np.frombuffer(raw[24:32], dtype="<i8")[0])
    d = np.frombuffer(raw[48:48 + 48 * n], dtype="<f8").reshape(6, n)
    w = np.frombuffer(raw[48 + 48 * n:48 + 56 * n], dtype="<i4").reshape(2, n)
    return dict(zip(ARRAYS, [*d, *w]))


def _parse_stretch(raw):
    """the record's file: ((nx, ny, nz, reserved), n, (reserved2, reserved3), F [3, 3, n], e)"""
    assert raw[:8] == b"EKPNPSF1"
    dims = tuple(int(v) for v in np.frombuffer(raw[8:24], dtype="<i4"))
    n, r2, r3 = (int(v) for v in np.frombuffer(raw[24:48], dtype="<i8"))
    assert len(raw) == 48 + 76 * n, (len(raw), n)
    e = np.frombuffer(raw[48:48 + 4 * n], dtype="<i4")
    F = np.frombuffer(raw[48 + 4 * n:], dtype="<f8").reshape(3, 3, n)
    return dims, n, (r2, r3), F, e


def _assert_cloud(got, want, what):
    for k, name in enumerate(("x", "y", "z")):
        assert T.same(got[k], want[k]), (what, name, np.flatnonzero(T.bits(got[k]) != T.bits(want[k]))[:5])
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]), what


def _assert_record(got, want, what):
    """F on its bit pattern (NaN where the host has NaN) and e"""
    assert got[0].shape == np.asarray(want[0]).shape and S.same_record(got, want), (
        what, np.argwhere(T.bits(got[0]) != T.bits(want[0]))[:5], np.flatnonzero(np.asarray(got[1]) != np.asarray(want[1]))[:5])


def _tangent(s, nsub, mu):
    s.tracers_advance(T.substep(s.p), nsub=nsub, mu=mu, stretch=True)


# ---- 1. the device equals the definition -----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["W", "O", "R", "T"])
def test_device_tangent_advance_equals_the_host_definition(pkg, inputs, host, shape, tmp_path):
    u, E, x, y, z = inputs[shape]
    p = _params(pkg, SHAPES[shape])
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        for n in NS:
            for nsub in NSUBS:
                for mu in (0.0, T.MU):
                    s.tracers_set(x[:n], y[:n], z[:n])
                    s.tracers_stretch_begin()
                    _tangent(s, nsub, mu)
                    s.tracers_save(str(tmp_path / "c.bin"), time=0.5)
                    cloud = _parse(open(tmp_path / "c.bin", "rb").read())
                    want = host(shape, n, nsub, mu)
                    what = (shape, n, nsub, mu)
                    for k, name in enumerate(("x", "y", "z")):
                        assert T.same(cloud[name], want[k]), (what, name)
                        assert T.same(cloud[name + "0"], (x, y, z)[k][:n]), (what, name + "0")
                    assert np.array_equal(cloud["wx"], want[3]) and np.array_equal(cloud["wy"], want[4]), what
                    _assert_record(s.tracers_stretch_get(), want[5:], what)
        # the cases did happen at n = 4097 after a hundred substeps: exponents raised, the lost particle's NaN rows, wraps, both plates
        want = host(shape, 4097, 100, T.MU)
        lost = np.isnan(want[0])
        assert lost[12] and np.isnan(want[5][:, :, 12]).all() and (want[6][~lost] > 0).sum() > 100
        want = host(shape, 4097, 7, T.MU)
        assert (want[3] != 0).any() and (want[4] != 0).any() and (want[2] == 0.0).any() and (want[2] == float(SHAPES[shape][2] - 1)).any()


def test_in_place_and_a_field_at_an_odd_address_give_the_same_bits(pkg, inputs, host):
    import torch

    u, E, x, y, z = inputs["W"]
    n = 1000
    with pkg.Solver(_params(pkg, SHAPES["W"], in_place=1)) as s:
        _put_fields(s, u, E)
        for mu in (0.0, T.MU):
            for nsub in (7, 100):
                s.tracers_set(x[:n], y[:n], z[:n])
                s.tracers_stretch_begin()
                _tangent(s, nsub, mu)
                want = host("W", n, nsub, mu)
                _assert_cloud(s.tracers_get(), want, ("in place", mu, nsub))
                _assert_record(s.tracers_stretch_get(), want[5:], ("in place", mu, nsub))
    with pkg.Solver(_params(pkg, SHAPES["W"])) as s:   # ux at an address that is 8 mod 16: the eight-byte loads of a stencil
        m = int(np.prod(s.shape))
        pool = torch.zeros(m + 3, dtype=torch.float64, device="cuda")
        view = pool[1:1 + m] if pool.data_ptr() % 16 == 0 else pool[2:2 + m]
        assert view.data_ptr() % 16 == 8
        s.bind_field("ux", view.data_ptr())
        _put_fields(s, u, E)
        for mu in (0.0, T.MU):
            s.tracers_set(x[:n], y[:n], z[:n])
            s.tracers_stretch_begin()
            _tangent(s, 7, mu)
            want = host("W", n, 7, mu)
            _assert_cloud(s.tracers_get(), want, ("bound", mu))
            _assert_record(s.tracers_stretch_get(), want[5:], ("bound", mu))
        off = (view.data_ptr() - pool.data_ptr()) // 8
        assert float(pool[:off].abs().sum()) == 0.0 and float(pool[off + m:].abs().sum()) == 0.0   # the guard elements are untouched


# ---- 2. / 3. the twin, and two calls ---------------------------------------------------------------------------------------

def test_the_cloud_moves_like_its_plain_twin_and_two_calls_equal_one(pkg, inputs, host):
    u, E, x, y, z = inputs["T"]
    p = _params(pkg, SHAPES["T"])
    n = 4097
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        for s in (a, b):
            _put_fields(s, u, E)
            s.tracers_set(x[:n], y[:n], z[:n])
        a.tracers_stretch_begin()
        for nsub, mu in ((3, T.MU), (4, T.MU)):
            _tangent(a, nsub, mu)
            b.tracers_advance(T.substep(p), nsub=nsub, mu=mu)
            _assert_cloud(a.tracers_get(), b.tracers_get(), ("the plain twin", nsub))
        first = ("T", n, 3, T.MU, None)
        host(*first[:4])
        want = host("T", n, 4, T.MU, first)
        _assert_cloud(a.tracers_get(), want, "3 + 4")
        _assert_record(a.tracers_stretch_get(), want[5:], "3 + 4")
        _assert_cloud(want, host("T", n, 7, T.MU), "two calls equal one")
        _assert_record(want[5:], host("T", n, 7, T.MU)[5:], "two calls equal one")
        # the other advances are allowed beside a record and leave it untouched
        before = a.tracers_stretch_get()
        a.tracers_advance(T.substep(p), nsub=2)
        a.tracers_advance(T.substep(p), nsub=1, D=1e-12, seed=3)
        a.tracers_advance(T.substep(p), nsub=1, D=1e-12, seed=3, absorb="top")
        _assert_record(a.tracers_stretch_get(), before, "plain, Brownian and absorbing advances")


# ---- 4. the sort ---------------------------------------------------------------------------------------------------------

def test_a_sorted_cloud_stretches_like_its_unsorted_twin(pkg, inputs, host):
    """the record is kept by slot and the sort permutes it: this fails if the sort leaves F or e behind"""
    u, E, x, y, z = inputs["T"]
    p = _params(pkg, SHAPES["T"])
    n = 4097   # one past the sort's run of 4096
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        for s in (a, b):
            _put_fields(s, u, E)
            s.tracers_set(x[:n], y[:n], z[:n])
            s.tracers_stretch_begin()
            _tangent(s, 3, T.MU)
        a.tracers_sort()
        ids = a.tracers_ids()
        assert (ids != np.arange(n)).sum() > n // 2   # the sort did move the particles
        Fa, ea = a.tracers_stretch_get()
        Fb, eb = b.tracers_stretch_get()
        _assert_record((Fa, ea), (Fb[:, :, ids], eb[ids]), "sorted: slot s holds particle ids[s]")
        _assert_record(a.tracers_stretch_get(by_id=True), (Fb, eb), "sorted, by id")
        for s in (a, b):
            _tangent(s, 4, T.MU)
        want = host("T", n, 7, T.MU)
        _assert_cloud(a.tracers_get(by_id=True), want, "sorted, then advanced")
        _assert_record(a.tracers_stretch_get(by_id=True), want[5:], "sorted, then advanced")
        _assert_record(b.tracers_stretch_get(), want[5:], "the twin")
        a.tracers_sort()   # a second sort composes
        assert not np.array_equal(a.tracers_ids(), ids)
        _assert_record(a.tracers_stretch_get(by_id=True), want[5:], "sorted twice")
        (ca, na), (cb, nb) = a.tracers_stretch_levels(-40, 64), b.tracers_stretch_levels(-40, 64)
        assert np.array_equal(ca, cb) and na == nb and ca.sum() + na == n   # a count does not care about the order
        ftle_a, det_a = a.tracers_ftle(7 * T.substep(p), by_id=True)
        ftle_b, det_b = b.tracers_ftle(7 * T.substep(p))
        assert T.same(ftle_a, ftle_b) and T.same(det_a, det_b) and np.isnan(ftle_b[12]) and np.isfinite(ftle_b[~np.isnan(want[0])]).all()


# ---- 5. the histogram of levels ------------------------------------------------------------------------------------------

def test_levels_equal_a_numpy_count_of_stretch_level(pkg, inputs, host):
    u, E, x, y, z = inputs["W"]
    p = _params(pkg, SHAPES["W"])
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        for n in (1, 4097, NBIG):
            s.tracers_set(x[:n], y[:n], z[:n])
            s.tracers_stretch_begin()
            counts, none = s.tracers_stretch_levels(0, 4)   # a record just begun: |I|^2 = 3, level 1; the lost one has none
            lost = int(np.isnan(x[:n]).sum())
            assert none == lost and counts[2] == n - lost and counts.sum() == n - lost
            _tangent(s, 100, T.MU)
            F, e = s.tracers_stretch_get()
            lv = np.atleast_1d(pkg.stretch_level(F, e))   # (an int for one particle)
            assert np.array_equal(lv, S.level(F, e))
            has = lv[lv != pkg.STRETCH_NO_LEVEL].astype(np.int64)
            assert has.size == n - np.isnan(s.tracers_get()[0]).sum()
            lo, hi, mid = (int(has.min()), int(has.max()), int(np.median(has))) if has.size else (0, 0, 0)
            if n > 1:
                assert hi - lo > 64
            for nlevels in (1, 64, 4096):
                for l_lo in ((mid, lo, hi - nlevels + 1, lo - 5, hi + 1) if n > 1 else (lo, lo - 3, lo + 1)):
                    counts, none = s.tracers_stretch_levels(l_lo, nlevels)
                    cell = np.clip(has - l_lo + 1, 0, nlevels + 1)
                    want = np.bincount(cell, minlength=nlevels + 2)
                    assert counts.dtype == np.int64 and counts.shape == (nlevels + 2,) and np.array_equal(counts, want) and none == n - has.size, (n, nlevels, l_lo)
                    assert np.array_equal(counts, S.levels_hist(F, e, l_lo, nlevels)[0])
                    if n > 1 and l_lo == mid and nlevels <= 64:
                        assert counts[0] > 0 and counts[-1] > 0   # the below and the above cell are both in use
        for kw, number in ((dict(l_lo=0, nlevels=0), "nlevels = 0"), (dict(l_lo=0, nlevels=4097), "nlevels = 4097")):
            with pytest.raises(pkg.EkpnpError) as e:
                s.tracers_stretch_levels(**kw)
            assert number in str(e.value) and "status 1" in str(e.value), kw
        # every particle in ONE cell, every lane of a wavefront at one counter
        s.tracers_stretch_begin()
        alive = NBIG - int(np.isnan(s.tracers_get()[0]).sum())   # (the hundred substeps lost some)
        counts, none = s.tracers_stretch_levels(1, 1)
        assert counts[1] == alive > NBIG // 2 and none == NBIG - alive and counts.sum() == alive
        assert s.tracers_stretch_levels(2 ** 31 - 5, 4096)[0][0] == alive and s.tracers_stretch_levels(-2 ** 31, 4096)[0][-1] == alive


# ---- 6. the record's life ------------------------------------------------------------------------------------------------

def test_save_both_files_load_both_and_continue_is_not_having_stopped(pkg, inputs, host, tmp_path):
    u, E, x, y, z = inputs["W"]
    p = _params(pkg, SHAPES["W"])
    cpath, spath = str(tmp_path / "cloud.bin"), str(tmp_path / "stretch.bin")
    n = 1000
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        _put_fields(a, u, E)
        _put_fields(b, u, E)
        a.tracers_set(x[:n], y[:n], z[:n])
        a.tracers_stretch_begin()
        _tangent(a, 45, T.MU)
        a.tracers_save(cpath, time=0.125)
        a.tracers_stretch_save(spath)
        raw = open(spath, "rb").read()
        assert os.path.getsize(cpath) == 48 + 56 * n   # the cloud's own file is unchanged
        dims, m, rest, F, e = _parse_stretch(raw)
        first = host("W", n, 45, T.MU)
        assert dims == (70, 66, 13, 0) and m == n and rest == (0, 0) and (e > 0).any()
        _assert_record((F, e), first[5:], "the file")
        assert b.tracers_load(cpath) == 0.125
        with pytest.raises(pkg.EkpnpError) as err:
            b.tracers_stretch_get()
        assert NO_RECORD in str(err.value)
        b.tracers_stretch_load(spath)
        _assert_record(b.tracers_stretch_get(), first[5:], "loaded")
        for s in (a, b):
            _tangent(s, 55, T.MU)
        want = host("W", n, 100, T.MU)
        for s in (a, b):
            _assert_cloud(s.tracers_get(), want, "continued")
            _assert_record(s.tracers_stretch_get(), want[5:], "continued")
        b.tracers_stretch_load(spath)   # a load replaces a record
        _assert_record(b.tracers_stretch_get(), first[5:], "replaced")

        def refused(name, edit, msg, s=b):
            bad = bytearray(raw)
            edit(bad)
            path = str(tmp_path / (name + ".bin"))
            open(path, "wb").write(bytes(bad))
            with pytest.raises(pkg.EkpnpError) as e:
                s.tracers_stretch_load(path)
            assert msg in str(e.value) and "status 1" in str(e.value), (name, str(e.value))

        def put(at, dtype, v):
            def edit(bad):
                bad[at:at + np.dtype(dtype).itemsize] = np.array([v], dtype).tobytes()
            return edit

        def cut(bad):
            del bad[-4:]

        refused("magic", put(0, "<i8", 7), "not a stretch file (EKPNPSF1)")
        refused("lattice", put(8, "<i4", 71), "lattice 71 x 66 x 13, not of 70 x 66 x 13")
        refused("count", put(24, "<i8", n + 1), "n = %d in the stretch file, the cloud has %d" % (n + 1, n))
        refused("short", cut, "shorter than its %d entries" % n)
        refused("reserved", put(20, "<i4", 2), "reserved = 2")
        refused("reserved2", put(32, "<i8", 5), "reserved = 0, 5, 0")
        _assert_record(b.tracers_stretch_get(), first[5:], "refused loads")
        b.tracers_release()
        refused("no cloud", lambda bad: None, "no cloud")


SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)


def _seeded_start(pkg, s):
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


def test_the_record_is_made_reset_dropped_and_freed_and_the_run_is_left_alone(pkg, tmp_path):
    """7. as well: a twin that never begins a record has the same device bytes and, after 4 real steps, the same fields"""
    p = _params(pkg, SHAPES["R"])
    n = 1000
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        _seeded_start(pkg, a)
        _seeded_start(pkg, b)
        a.step(5)
        b.step(5)
        state = a.graph_state()
        before = a.device_bytes()
        a.tracers_seed(n=n, seed=1)
        with_cloud = a.device_bytes()

        def absent():
            for call in (lambda: a.tracers_stretch_get(), lambda: a.tracers_advance(p.dt, stretch=True), lambda: a.tracers_stretch_levels(0, 4),
                         lambda: a.tracers_stretch_save(str(tmp_path / "none.bin"))):
                with pytest.raises(pkg.EkpnpError) as e:
                    call()
                assert NO_RECORD in str(e.value) and "status 1" in str(e.value)
            assert a.device_bytes() == with_cloud

        absent()
        a.tracers_stretch_end()   # nothing to drop
        a.tracers_advance(p.dt, nsub=2)
        absent()
        a.tracers_stretch_begin()
        assert a.device_bytes() == with_cloud + 76 * n
        for k in range(4):
            a.step(1)
            a.tracers_advance(p.dt, nsub=2, mu=1e-8 if k % 2 else 0.0, stretch=True)
            assert a.device_bytes() == with_cloud + 76 * n
        F, e = a.tracers_stretch_get()
        ident = pkg.stretch_identity(*a.tracers_get()[:3])[0]
        assert not np.array_equal(F, ident) and np.abs(F - ident).max() < 0.5 and not e.any()
        a.tracers_stretch_begin()   # begin again: reset
        F, e = a.tracers_stretch_get()
        assert np.array_equal(F, ident) and not e.any() and a.device_bytes() == with_cloud + 76 * n
        a.tracers_stretch_levels(0, 4)
        with_table = a.device_bytes()
        assert with_table == with_cloud + 76 * n + 8 * (pkg.TRACERS_MAX_CELLS + 1)   # the table of the cell counts, shared
        # seed, set and load drop it; so does end
        a.tracers_save(str(tmp_path / "c.bin"))
        x, y, z = a.tracers_get()[:3]
        for renew in (lambda: a.tracers_seed(n=n, seed=2), lambda: a.tracers_set(x, y, z), lambda: a.tracers_load(str(tmp_path / "c.bin")), lambda: a.tracers_stretch_end()):
            a.tracers_stretch_begin()
            a.tracers_advance(p.dt, stretch=True)
            assert a.device_bytes() == with_table
            renew()
            assert a.device_bytes() == with_table - 76 * n
            with pytest.raises(pkg.EkpnpError) as e:
                a.tracers_stretch_get()
            assert NO_RECORD in str(e.value)
        a.tracers_stretch_begin()
        a.tracers_seed(n=2 * n, seed=2)   # another size: dropped with the cloud it belonged to
        with pytest.raises(pkg.EkpnpError) as e:
            a.tracers_stretch_get()
        assert NO_RECORD in str(e.value)
        a.tracers_stretch_begin()
        assert a.tracers_stretch_get()[1].size == 2 * n
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
    s.tracers_advance(1e-9, nsub=2, D=1e-9, absorb="both")
    s.tracers_sort(); s.tracers_moments(); s.tracers_cell_counts((4, 3, 2)); s.tracers_sample(["ux"]); s.tracers_save(sys.argv[1])
    print("PLAIN OK", s.tracers_epoch(), cloud, s.device_bytes() - before)
    s.tracers_stretch_begin()
    try:
        s.tracers_advance(1e-9, nsub=2, stretch=True)
        print("TANGENT OK")
    except pkg.EkpnpError as e:
        print("ERR", e)
''' % ROOT


def test_a_context_that_never_begins_a_record_launches_no_tangent_kernel_and_allocates_nothing(tmp_path):
    """the library's launch-failure knob (read once per process, hence a child) fails the named kernel's first launch: everything a
    cloud did before this change goes through with the bytes it had - the cloud 56 n + its partials, the landing record 36 n, the
    sort's scratch 16 n + tables, the ids 4 n, the cell table, the sample scratch 8 n - and the tangent advance reports that kernel
    by name"""
    env = dict(os.environ, EKPNP_INJECT_LAUNCH_FAILURE="k_tracers_advance_tangent")
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "c.bin")], env=env, capture_output=True, text=True, timeout=300)
    n = 5000
    cloud, rest = 56 * n + 3 * 12 * 8, 36 * n + (16 * n + 4 * (256 * 2 + 1)) + 4 * n + 8 * 65537 + 8 * n
    assert r.returncode == 0 and "PLAIN OK 4 %d %d" % (cloud, rest) in r.stdout and "ERR" in r.stdout and "kernel k_tracers_advance_tangent:" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert os.path.getsize(tmp_path / "c.bin") == 48 + 60 * n


# ---- 8. refusals -------------------------------------------------------------------------------------------------------

def test_refusals_of_the_context_calls(pkg, tmp_path):
    p = _params(pkg, SHAPES["W"])
    msg = "tracers: slab contexts are not supported"
    for rank, nranks in ((0, 1), (1, 3)):
        with pkg.Solver(p, rank=rank, nranks=nranks, slab=True) as s:
            calls = (lambda: s.tracers_stretch_begin(), lambda: s.tracers_stretch_end(), lambda: s.tracers_advance(1e-9, stretch=True), lambda: s.tracers_stretch_get(),
                     lambda: s.tracers_stretch_levels(0, 4), lambda: s.tracers_stretch_save(str(tmp_path / "x.bin")), lambda: s.tracers_stretch_load(str(tmp_path / "x.bin")))
            for k, call in enumerate(calls):
                with pytest.raises(pkg.EkpnpError) as e:
                    call()
                assert "status 1" in str(e.value) and msg in str(e.value), k
    assert not [m for m in dir(pkg.Group) if "tracers" in m or "stretch" in m]   # and a group has no spelling of them
    with pkg.Solver(p) as s:
        for call in (lambda: s.tracers_stretch_begin(), lambda: s.tracers_advance(1e-9, stretch=True), lambda: s.tracers_stretch_levels(0, 4),
                     lambda: s.tracers_stretch_save(str(tmp_path / "x.bin")), lambda: s.tracers_stretch_load(str(tmp_path / "x.bin"))):
            with pytest.raises(pkg.EkpnpError) as e:
                call()
            assert "no cloud" in str(e.value)
        s.tracers_stretch_end()   # no cloud, no record: nothing to drop
        s.tracers_seed(n=100, seed=1)
        with pytest.raises(pkg.EkpnpError) as e:
            s.tracers_advance(1e-9, stretch=True)   # without a record
        assert NO_RECORD in str(e.value) and "status 1" in str(e.value)
        s.tracers_stretch_begin()
        before, rec = s.tracers_get(), s.tracers_stretch_get()
        for kw, number in ((dict(h=1e-9, nsub=0), "nsub = 0"), (dict(h=1e-9, nsub=4097), "nsub = 4097"), (dict(h=float("inf")), "h = inf"),
                           (dict(h=1e-9, mu=float("inf")), "mu = inf"), (dict(h=float("nan")), "h = nan")):
            with pytest.raises(pkg.EkpnpError) as e:
                s.tracers_advance(stretch=True, **kw)
            assert number in str(e.value) and "status 1" in str(e.value), kw
        for kw in (dict(D=1e-9), dict(D=0.0), dict(absorb="both"), dict(D=1e-9, absorb="top")):
            with pytest.raises(ValueError):
                s.tracers_advance(1e-9, stretch=True, **kw)
        _assert_cloud(s.tracers_get(), before, "refused")   # a refused call moves nobody
        _assert_record(s.tracers_stretch_get(), rec, "refused")


# ---- 9. the driver -----------------------------------------------------------------------------------------------------

def _run_driver(args, out, code=0):
    out.mkdir()
    env = dict(os.environ, EKPNP_PLACEMENT_TRIES="1")  # the child shares device 0 with this process
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == code, (args, r.stderr[-2000:])
    return out, r.stderr


GEO = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "6", "--seed-pattern", "squares", "--seed-modes", "1,1"]


def test_driver_writes_the_stretch_files_of_the_library_calls_in_both_loops(pkg, tmp_path):
    assert os.path.exists(EXE), "ekpnp_main not built"
    p = pkg.default_params(40, 12, 17)
    mu = 1e-9
    spec = pkg.tracers_spec(n=1000, box=((0, 40), (0, 12), (1, 15)), seed=9)
    with pkg.Solver(p) as s:  # the driver's loop, call by call
        s.initialization()
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-3, noise=0.0, relative=True, seed=1))
        s.fast_Poisson()
        s.init_equilibrium()
        s.tracers_seed(spec)
        s.tracers_stretch_begin()
        t = 0.0
        for i in range(6):
            s.stream_collide_save(t)
            s.fast_Poisson()
            t = t + p.dt
            if (i + 1) % 2 == 0:
                s.tracers_advance(2.0 * p.dt, nsub=3, mu=mu, stretch=True)
        s.tracers_stretch_save(str(tmp_path / "lib_stretch.bin"))
        s.tracers_save(str(tmp_path / "lib_cloud.bin"), time=t)
        F, e = s.tracers_stretch_get()
        counts, none = s.tracers_stretch_levels(-2, 8)
    flags = ["--tracers", "1000", "--tracers-box", "0,40,0,12,1,15", "--tracers-seed", "9", "--tracers-every", "2", "--tracers-substeps", "3", "--tracers-mobility", "1e-9",
             "--tracers-stretch", "--stretch-levels", "-2,8"]
    loop, _ = _run_driver([*GEO, *flags], tmp_path / "loop")
    batch, _ = _run_driver([*GEO, *flags, "--batch", "1"], tmp_path / "batch")
    for f in ("stretch.bin", "stretch_levels.dat", "tracers.dat", "tracers_final.bin"):
        v = (loop / f).read_bytes()
        assert len(v) > 0 and v == (batch / f).read_bytes(), f
    assert (loop / "stretch.bin").read_bytes() == (tmp_path / "lib_stretch.bin").read_bytes()
    assert (loop / "tracers_final.bin").read_bytes()[48:] == (tmp_path / "lib_cloud.bin").read_bytes()[48:]   # (the header holds the time)
    dims, n, rest, gF, ge = _parse_stretch((loop / "stretch.bin").read_bytes())
    assert dims == (40, 12, 17, 0) and n == 1000 and rest == (0, 0)
    _assert_record((gF, ge), (F, e), "stretch.bin")
    assert not np.array_equal(gF, pkg.stretch_identity(np.zeros(n), np.zeros(n), np.zeros(n))[0])
    lines = (loop / "stretch_levels.dat").read_text().splitlines()
    assert lines[0].startswith("# ekpnp stretch levels nx 40 ny 12 nz 17 n 1000 l_lo -2 nlevels 8") and len(lines) == 2
    assert [int(v) for v in lines[1].split(" ")] == [none, *counts] and counts.sum() + none == 1000
    # without --stretch-levels: the record's file alone; and the refusals of the flags
    plain, _ = _run_driver([*GEO, "--tracers", "100", "--tracers-stretch"], tmp_path / "plain")
    assert _parse_stretch((plain / "stretch.bin").read_bytes())[1] == 100 and not (plain / "stretch_levels.dat").exists()
    for k, (bad, number) in enumerate(((["--tracers-stretch"], "there is no cloud to stretch"), (["--tracers", "10", "--stretch-levels", "0,4"], "nothing is stretched"),
                                       (["--tracers", "10", "--tracers-stretch", "--tracers-diffusivity", "1e-9"], "deterministic advance only"),
                                       (["--tracers", "10", "--tracers-stretch", "--tracers-absorb", "top"], "deterministic advance only"),
                                       (["--tracers", "10", "--tracers-stretch", "--stretch-levels", "0,5000"], "got 0,5000"),
                                       (["--tracers", "10", "--tracers-stretch", "--stretch-levels", "4"], "got 4"))):
        _, err = _run_driver([*GEO, *bad], tmp_path / ("bad%d" % k), code=2)
        assert number in err, err
