"""GPU tests of the Lagrangian tracers (csrc/tracers.hip; include/ekpnp.h: ekpnp_tracers_*; `ekpnp_main --tracers N`).

The host functions are the definitions (tests/test_tracers_cpu.py holds them against a numpy transcription), so the device is compared
with them on the float64 BIT PATTERN: positions, image counts and which particles are lost.  Counts are integers and compared exactly.
The one toleranced check is the moments' sums on random displacements, with the a-priori bound n * 2^-53 * sum|term| of any order of
n additions.  Shapes: W 70 x 66 x 13, O 35 x 33 x 5 (odd: the planes start at odd doubles), R 40 x 12 x 17; n = 1 (one lane), 1000 (not a
multiple of 256), 4097 (one particle past the moments' run of 4096: two workgroups of partial sums)."""
import math
import os
import subprocess

import numpy as np
import pytest

import _tracers_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
W = (70, 66, 13)
O = (35, 33, 5)
R = (40, 12, 17)
SHAPES = {"W": W, "O": O, "R": R}
UE = ("ux", "uy", "uz", "Ex", "Ey", "Ez")


def _params(pkg, shape, in_place=0):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    p.in_place = in_place
    return p


@pytest.fixture(scope="module")
def inputs(pkg):
    """per shape: (u, E) random fields and a cloud of 4097 positions whose first 13 hold the special ones; made once, never modified"""
    out = {}
    for k, s in SHAPES.items():
        u, E = T.random_fields(s, 81 + len(out), T.U_SCALE, T.E_SCALE)
        x, y, z = T.special_cloud(s, 4097, 91 + len(out))
        for a in (*u, *E, x, y, z):
            a.setflags(write=False)
        out[k] = (u, E, x, y, z)
    return out


def _put_fields(s, u, E):
    for name, a in zip(UE, (*u, *E)):
        s.set_field(name, a)


def _assert_cloud(got, want, what):
    for k, name in enumerate(("x", "y", "z")):
        assert T.same(got[k], want[k]), (what, name, np.flatnonzero(T.bits(got[k]) != T.bits(want[k]))[:5])
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]), what


COMBOS = [(n, nsub, mu) for n in (1, 1000, 4097) for nsub in (1, 7) for mu in (0.0, T.MU)]


@pytest.fixture(scope="module")
def host_advance(pkg, inputs):
    """host_advance(shape, n, nsub, mu, sign) -> ekpnp_tracers_advance_host of the first n particles; computed once per case"""
    cache = {}

    def get(shape, n, nsub, mu, sign=1.0):
        key = (shape, n, nsub, mu, sign)
        if key not in cache:
            u, E, x, y, z = inputs[shape]
            p = pkg.default_params(*SHAPES[shape])
            cache[key] = pkg.tracers_advance_host(p, u, x[:n], y[:n], z[:n], E=E, mu=mu, h=sign * T.substep(p), nsub=nsub)
            for a in cache[key]:
                a.setflags(write=False)
        return cache[key]

    return get


# ---- 1. the advance ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["W", "O", "R"])
def test_device_advance_equals_advance_host(pkg, inputs, host_advance, shape):
    u, E, x, y, z = inputs[shape]
    p = _params(pkg, SHAPES[shape])
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        for n, nsub, mu in COMBOS:
            s.tracers_set(x[:n], y[:n], z[:n])
            assert s.tracers_size == n
            s.tracers_advance(T.substep(p), nsub=nsub, mu=mu)
            got = s.tracers_get()
            want = host_advance(shape, n, nsub, mu)
            _assert_cloud(got, want, (shape, n, nsub, mu))
            if n >= 1000:
                assert np.isnan(got[0][12]) and np.isnan(got[0]).sum() == np.isnan(want[0]).sum()
        # backwards in time, and a second call continues the first
        s.tracers_set(x[:1000], y[:1000], z[:1000])
        s.tracers_advance(-T.substep(p), nsub=7, mu=T.MU)
        _assert_cloud(s.tracers_get(), host_advance(shape, 1000, 7, T.MU, -1.0), (shape, "backwards"))
        s.tracers_set(x[:1000], y[:1000], z[:1000])
        for _ in range(7):
            s.tracers_advance(T.substep(p), nsub=1, mu=0.0)
        _assert_cloud(s.tracers_get(), host_advance(shape, 1000, 7, 0.0), (shape, "call by call"))
        wx = s.tracers_get()[3]
        assert (wx > 0).any() and (wx < 0).any()


def test_in_place_and_a_bound_array_give_the_same_bits(pkg, inputs, host_advance):
    import torch

    u, E, x, y, z = inputs["W"]
    with pkg.Solver(_params(pkg, W, in_place=1)) as s:
        _put_fields(s, u, E)
        p = s.p
        for mu in (0.0, T.MU):
            s.tracers_set(x[:1000], y[:1000], z[:1000])
            s.tracers_advance(T.substep(p), nsub=7, mu=mu)
            _assert_cloud(s.tracers_get(), host_advance("W", 1000, 7, mu), ("in place", mu))
    with pkg.Solver(_params(pkg, W)) as s:  # ux at an address that is 8 mod 16
        n = int(np.prod(s.shape))
        pool = torch.zeros(n + 3, dtype=torch.float64, device="cuda")
        view = pool[1:1 + n] if pool.data_ptr() % 16 == 0 else pool[2:2 + n]
        assert view.data_ptr() % 16 == 8
        s.bind_field("ux", view.data_ptr())
        _put_fields(s, u, E)
        for mu in (0.0, T.MU):
            s.tracers_set(x[:1000], y[:1000], z[:1000])
            s.tracers_advance(T.substep(s.p), nsub=7, mu=mu)
            _assert_cloud(s.tracers_get(), host_advance("W", 1000, 7, mu), ("bound", mu))
        s.synchronize()
        off = (view.data_ptr() - pool.data_ptr()) // 8
        assert float(pool[:off].abs().sum()) == 0.0 and float(pool[off + n:].abs().sum()) == 0.0  # the guard elements are untouched


SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)


def _seeded_start(pkg, s, **knobs):
    for k, v in knobs.items():
        s.tune(k, v)
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


def test_after_real_steps_the_advance_reads_the_fields_get_field_returns(pkg):
    """lazy E is on: after step(3) the E arrays are older than phi.  A charged advance must bring them up to date first (it then
    equals advance_host on what a twin's get_field returns); a passive one reads u only, and the run goes on as the twin's."""
    p = _params(pkg, R)
    spec = pkg.tracers_spec(n=1000, p=p, seed=3)
    x0, y0, z0 = pkg.tracers_seed_host(p, spec)
    with pkg.Solver(p) as a, pkg.Solver(p) as b, pkg.Solver(p) as c:
        for s in (a, b, c):
            _seeded_start(pkg, s)
            s.step(3)
        f = c.fields()
        u, E = [f[k] for k in UE[:3]], [f[k] for k in UE[3:]]
        assert max(np.abs(v).max() for v in u) > 0.0 and max(np.abs(v).max() for v in E) > 0.0
        # large steps, so that the tiny velocities of a young flow move the particles by cells: mu sized so that mu E is a cell per substep
        h = 0.5 * p.dx / max(np.abs(v).max() for v in u)
        mu = 0.5 * max(np.abs(v).max() for v in u) / max(np.abs(v).max() for v in E)
        a.tracers_seed(spec)
        a.tracers_advance(h, nsub=5, mu=mu)
        want = pkg.tracers_advance_host(p, u, x0, y0, z0, E=E, mu=mu, h=h, nsub=5)
        _assert_cloud(a.tracers_get(), want, "charged")
        passive = pkg.tracers_advance_host(p, u, x0, y0, z0, mu=0.0, h=h, nsub=5)
        assert not T.same(passive[0], want[0])
        moved = max(np.nanmax(np.abs(w - w0)) for w, w0 in zip(want[:3], (x0, y0, z0)))
        print(f"h {h:.3e} s, mu {mu:.3e}, largest displacement {moved:.3f} cells, lost {int(np.isnan(want[0]).sum())}")
        assert moved > 0.05 and np.isnan(want[0]).sum() < 100
        b.tracers_seed(spec)
        b.tracers_advance(h, nsub=5, mu=0.0)   # lazy E is left alone: nothing but u is read
        for s in (a, b, c):
            s.step(3)
        _assert_cloud(b.tracers_get(), passive, "passive")
        fa, fb, fc = a.fields(), b.fields(), c.fields()
        for n in pkg.FIELDS:
            assert np.array_equal(T.bits(fa[n]), T.bits(fc[n])) and np.array_equal(T.bits(fb[n]), T.bits(fc[n])), n


# ---- 2. seeding, set and get --------------------------------------------------------------------------------------------

def test_device_seed_equals_seed_host(pkg):
    p = _params(pkg, W)
    specs = [pkg.tracers_spec(n=1000, p=p, seed=7), pkg.tracers_spec(n=4097, box=((3.25, 3.5), (65.0, 66.0), (0.0, 12.0)), seed=2 ** 63 + 11),
             pkg.tracers_spec(grid=(7, 11, 13), p=p), pkg.tracers_spec(grid=(70, 3, 1), box=((0, 70), (0, 66), (0, 12))), pkg.tracers_spec(n=1, p=p)]
    with pkg.Solver(p) as s:
        for spec in specs:
            s.tracers_seed(spec)
            assert s.tracers_size == spec.n
            x, y, z, wx, wy = s.tracers_get()
            hx, hy, hz = pkg.tracers_seed_host(p, spec)
            assert T.same(x, hx) and T.same(y, hy) and T.same(z, hz), (spec.mode, spec.n)
            assert not wx.any() and not wy.any()
            m = s.tracers_moments()
            assert m[0] == spec.n and not m[1:8].any()  # start positions are the positions
        with pytest.raises(pkg.EkpnpError) as e:
            s.tracers_seed(pkg.tracers_spec(n=61, grid=(5, 4, 3), p=p))
        assert "5*4*3" in str(e.value)


def test_set_refuses_a_position_outside_and_get_returns_what_was_set(pkg, inputs):
    u, E, x, y, z = inputs["W"]
    with pkg.Solver(_params(pkg, W)) as s:
        assert s.tracers_size == 0
        with pytest.raises(pkg.EkpnpError) as e:
            s.tracers_get()
        assert "no cloud" in str(e.value)
        with pytest.raises(pkg.EkpnpError):
            s.tracers_advance(1e-9)
        s.tracers_set(x[:1000], y[:1000], z[:1000])
        got = s.tracers_get()
        assert T.same(got[0], x[:1000]) and T.same(got[1], y[:1000]) and T.same(got[2], z[:1000]) and not got[3].any() and not got[4].any()
        for k, (bx, by, bz) in ((0, (70.0, 1.0, 1.0)), (5, (1.0, -1e-300, 1.0)), (999, (1.0, 1.0, 12.5)), (17, (np.nan, 1.0, 1.0)), (3, (np.inf, 1.0, 1.0))):
            xx, yy, zz = x[:1000].copy(), y[:1000].copy(), z[:1000].copy()
            xx[k], yy[k], zz[k] = bx, by, bz
            with pytest.raises(pkg.EkpnpError) as e:
                s.tracers_set(xx, yy, zz)
            assert f"particle {k} " in str(e.value) and "status 1" in str(e.value)
        assert T.same(s.tracers_get()[0], x[:1000])  # a refused set leaves the cloud alone
        s.tracers_release()
        assert s.tracers_size == 0


# ---- 3. cell counts ----------------------------------------------------------------------------------------------------

def test_cell_counts_equal_bincount_of_the_host_cell_function(pkg, inputs):
    u, E, x, y, z = inputs["W"]
    p = _params(pkg, W)
    with pkg.Solver(p) as s:
        x2, y2, z2 = x.copy(), y.copy(), z.copy()
        x2[100:140] = y2[100:140] = z2[100:140] = np.nan   # more lost ones
        s.tracers_set(x2, y2, z2)
        # 1 cell; tables in LDS up to 63 x 13 x 10 = 8190 cells (+ lost: 8191 of 8192 counters); 64 x 16 x 8 = 8192 cells is the first in global memory
        for cells in ((1, 1, 1), (4, 3, 2), (16, 16, 12), (70, 66, 1), (63, 13, 10), (64, 16, 8), (64, 64, 12), (64, 32, 12)):
            counts, lost = s.tracers_cell_counts(cells)
            c = T.cell(W, cells, x2, y2, z2)
            want = np.bincount(c[c >= 0], minlength=cells[0] * cells[1] * cells[2]).reshape(cells[2], cells[1], cells[0])
            assert counts.dtype == np.int64 and np.array_equal(counts, want), cells
            assert lost == 41 and counts.sum() + lost == 4097
        # all particles in one cell: every lane of every wavefront adds to one counter
        n = 4097
        rng = np.random.default_rng(5)
        s.tracers_set(20.0 + rng.uniform(0, 1, n), 30.0 + rng.uniform(0, 1, n), 6.0 + rng.uniform(0, 1, n))
        for cells in ((70, 66, 12), (7, 6, 4), (1, 1, 1)):
            counts, lost = s.tracers_cell_counts(cells)
            assert lost == 0 and counts.max() == n and counts.sum() == n and np.count_nonzero(counts) == 1
            assert counts[(6 * cells[2]) // 12, (30 * cells[1]) // 66, (20 * cells[0]) // 70] == n
        for cells, number in (((71, 1, 1), "bx = 71"), ((1, 0, 1), "by = 0"), ((1, 1, 13), "bz = 13"), ((70, 66, 12 + 3), "bz = 15")):
            with pytest.raises(pkg.EkpnpError) as e:
                s.tracers_cell_counts(cells)
            assert number in str(e.value)
    big = (64, 64, 17)
    with pkg.Solver(_params(pkg, big)) as s:   # bx*by*bz of exactly 65536, and one more refused
        spec = pkg.tracers_spec(n=4097, box=((0, 64), (0, 64), (0, 16)), seed=4)
        s.tracers_seed(spec)
        hx, hy, hz = pkg.tracers_seed_host(s.p, spec)
        counts, lost = s.tracers_cell_counts((64, 64, 16))
        c = T.cell(big, (64, 64, 16), hx, hy, hz)
        assert lost == 0 and np.array_equal(counts.ravel(), np.bincount(c, minlength=65536))
        assert np.array_equal(pkg.tracers_cell(s.p, (64, 64, 16), hx[:200], hy[:200], hz[:200]), c[:200])
        with pytest.raises(pkg.EkpnpError) as e:
            s.tracers_cell_counts((64, 64, 17))
        assert "bz = 17" in str(e.value)


# ---- 4. moments --------------------------------------------------------------------------------------------------------

def _moment_terms(shape, x0, y0, z0, x, y, z, wx, wy):
    """the terms of the ten sums of the alive particles, as the header forms them"""
    alive = ~np.isnan(x)
    dx = (x[alive] - x0[alive]) + wx[alive].astype(np.float64) * float(shape[0])
    dy = (y[alive] - y0[alive]) + wy[alive].astype(np.float64) * float(shape[1])
    dz = z[alive] - z0[alive]
    za = z[alive]
    return alive, [dx, dy, dz, dx * dx, dy * dy, dz * dz, za, za * za]


def test_moments_are_exact_on_dyadic_displacements(pkg):
    p = _params(pkg, W)
    p.dx = p.dy = p.dz = 2.0 ** -17
    nz, ny, nx = W[2], W[1], W[0]
    n = 4097
    rng = np.random.default_rng(11)
    x0 = rng.integers(0, nx * 8, n) / 8.0
    y0 = rng.integers(0, ny * 8, n) / 8.0
    z0 = rng.integers(0, (nz - 1) * 8 + 1, n) / 8.0
    x0[7] = y0[7] = z0[7] = np.nan
    x0[4096] = y0[4096] = z0[4096] = np.nan
    u = [np.full((nz, ny, nx), 0.375 / 128.0), np.full((nz, ny, nx), -0.25 / 128.0), np.zeros((nz, ny, nx))]
    with pkg.Solver(p) as s:
        _put_fields(s, u, [np.zeros((nz, ny, nx))] * 3)
        s.tracers_set(x0, y0, z0)
        s.tracers_advance(2.0 ** -10, nsub=8 * 40)   # 120 cells along x: every particle wraps at least once
        m = s.tracers_moments()
        x, y, z, wx, wy = s.tracers_get()
    alive = ~np.isnan(x0)
    assert wx[alive].min() >= 1 and wy[alive].max() <= -1 and not wx[~alive].any()
    zs = z0[alive]
    want = [n - 2, 2, 120.0 * (n - 2), -80.0 * (n - 2), 0.0, 14400.0 * (n - 2), 6400.0 * (n - 2), 0.0, zs.sum(), (zs * zs).sum(), zs.min(), zs.max()]
    assert m.tolist() == want  # every term and every partial sum is a small dyadic number: exact in any order
    assert np.isnan(x[7]) and np.isnan(x[4096]) and T.same(z[alive], zs)


def test_moments_on_random_displacements_lie_within_the_a_priori_bound(pkg, inputs, host_advance):
    u, E, x0, y0, z0 = inputs["W"]
    p = _params(pkg, W)
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        for n in (1, 1000, 4097):
            s.tracers_set(x0[:n], y0[:n], z0[:n])
            s.tracers_advance(T.substep(p), nsub=7, mu=T.MU)
            m = s.tracers_moments()
            x, y, z, wx, wy = host_advance("W", n, 7, T.MU)
            alive, terms = _moment_terms(W, x0[:n], y0[:n], z0[:n], x, y, z, wx, wy)
            assert m[0] == alive.sum() and m[1] == n - alive.sum() and m[1] >= (1 if n >= 13 else 0)
            for k, t in enumerate(terms):
                tol = n * 2.0 ** -53 * np.abs(t).sum()
                d = abs(m[2 + k] - math.fsum(t))
                print(f"n {n} {pkg.TRACER_MOMENTS[2 + k]}: {d:.3e} (tol {tol:.3e})")
                assert d <= tol, (n, pkg.TRACER_MOMENTS[2 + k], d, tol)
            assert m[10] == z[alive].min() and m[11] == z[alive].max()   # min and max are exact
            if n >= 1000:
                assert np.abs(m[2:5]).max() > 1.0
        s.tracers_set([np.nan] * 3, [np.nan] * 3, [np.nan] * 3)   # nobody alive: +0.0 everywhere, z_min = z_max = 0
        m = s.tracers_moments()
        assert m.tolist() == [0.0, 3.0] + [0.0] * 10 and not np.signbit(m).any()


# ---- 5. the ring -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride, batch, charged", [(1, 0, False), (3, 0, True), (1, 1, True), (3, 1, False)])
def test_ring_rows_equal_a_twins_synchronous_moments(pkg, stride, batch, charged, tmp_path):
    p = _params(pkg, R)
    spec = pkg.tracers_spec(n=1000, p=p, seed=2)
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        _seeded_start(pkg, a, batch_moments=batch)
        _seeded_start(pkg, b)
        assert a.tracers_count() == (0, 0)
        with pytest.raises(pkg.EkpnpError):
            a.tracers_record(0, 0.0)   # nothing armed
        a.tracers_seed(spec)
        b.tracers_seed(spec)
        a.tracers_arm(capacity=4)
        a.step(2)
        b.step(2)
        # a young flow is slow: a substep sized from the twin's fields, so that the fastest node moves a particle a quarter of a cell
        umax = max(np.abs(b.get_field(k)).max() for k in UE[:3])
        emax = max(np.abs(b.get_field(k)).max() for k in UE[3:])
        assert umax > 0.0 and emax > 0.0
        h = 0.25 * p.dx / umax
        mu = 0.25 * umax / emax if charged else 0.0
        want = []
        for k in range(1, 7):
            a.step(stride)
            a.tracers_advance(h, nsub=2, mu=mu)
            a.tracers_record(k * stride, a.t)
            b.step(stride)
            b.tracers_advance(h, nsub=2, mu=mu)
            want.append((k * stride, b.t, b.tracers_moments()))
        assert a.tracers_count() == (6, 2)   # the ring held four: the two oldest rows are gone
        steps, times, rows = a.tracers_read()
        assert rows.shape == (4, 12)
        assert steps.tolist() == [w[0] for w in want[2:]] and times.tolist() == [w[1] for w in want[2:]]
        for row, w in zip(rows, want[2:]):
            assert T.same(row, w[2]), w[0]
        print(rows[0], rows[-1])
        assert rows[0][0] + rows[0][1] == 1000 and rows[-1][0] > 500 and (T.bits(rows[-1]) != T.bits(rows[0])).any()
        s1, _, r1 = a.tracers_read(1, 2)
        assert s1.tolist() == steps[1:3].tolist() and T.same(r1, rows[1:3])
        for first, count in ((2, 3), (-1, 1), (4, 1)):
            with pytest.raises(pkg.EkpnpError) as e:
                a.tracers_read(first, count)
            assert "status 1" in str(e.value)
        a.tracers_ring_save(str(tmp_path / "ring.dat"))
        lines = open(tmp_path / "ring.dat").read().splitlines()
        assert lines[0] == "# ekpnp tracers nx 40 ny 12 nz 17 n 1000 recorded 6 dropped 2"
        assert lines[1] == "# step time " + " ".join(pkg.TRACER_MOMENTS) and len(lines) == 6
        for ln, st, tm, row in zip(lines[2:], steps, times, rows):
            w = ln.split(" ")
            assert int(w[0]) == st and float(w[1]) == tm and T.same(np.array([float(v) for v in w[2:]]), row)   # %.17g round-trips
        a.tracers_disarm()
        assert T.same(a.tracers_read()[2], rows)
        with pytest.raises(pkg.EkpnpError):
            a.tracers_record(7, 0.0)
        with pytest.raises(pkg.EkpnpError) as e:
            a.tracers_arm(capacity=0)
        assert "capacity = 0" in str(e.value)
        a.tracers_arm(capacity=3)
        assert a.tracers_count() == (0, 0) and a.tracers_read()[2].shape == (0, 12)


# ---- 6. the cloud's file -----------------------------------------------------------------------------------------------

def test_save_load_and_continue_is_bit_for_bit(pkg, inputs, tmp_path):
    u, E, x, y, z = inputs["W"]
    p = _params(pkg, W)
    h = T.substep(p)
    path = str(tmp_path / "cloud.bin")
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        _put_fields(a, u, E)
        _put_fields(b, u, E)
        a.tracers_set(x[:1000], y[:1000], z[:1000])
        a.tracers_advance(h, nsub=3, mu=T.MU)
        a.tracers_save(path, time=0.125)
        raw = open(path, "rb").read()
        assert len(raw) == 48 + 1000 * 56 and raw[:8] == b"EKPNPTR1"
        assert np.frombuffer(raw[8:24], dtype="<i4").tolist() == [70, 66, 13, 0] and np.frombuffer(raw[24:32], dtype="<i8")[0] == 1000
        assert np.frombuffer(raw[32:40], dtype="<f8")[0] == 0.125
        got = a.tracers_get()
        body = np.frombuffer(raw[48:48 + 6000 * 8], dtype="<f8").reshape(6, 1000)
        assert T.same(body[0], got[0]) and T.same(body[2], got[2]) and T.same(body[3], x[:1000]) and T.same(body[5], z[:1000])
        assert np.array_equal(np.frombuffer(raw[48 + 48000:], dtype="<i4").reshape(2, 1000), np.stack(got[3:5]))
        assert b.tracers_load(path) == 0.125 and b.tracers_size == 1000
        _assert_cloud(b.tracers_get(), got, "loaded")
        for s in (a, b):
            s.tracers_advance(h, nsub=4, mu=T.MU)
        _assert_cloud(b.tracers_get(), a.tracers_get(), "continued")
        assert T.same(b.tracers_moments(), a.tracers_moments())   # the start positions and image counts came along
        want = pkg.tracers_advance_host(p, u, x[:1000], y[:1000], z[:1000], E=E, mu=T.MU, h=h, nsub=7)
        _assert_cloud(b.tracers_get(), want, "as if it had not stopped")
        # refusals: a short file, a position outside, another lattice
        open(tmp_path / "short.bin", "wb").write(raw[:-4])
        bad = bytearray(raw)
        bad[48 + 8 * 20:48 + 8 * 21] = np.float64(70.0).tobytes()
        open(tmp_path / "outside.bin", "wb").write(bytes(bad))
        for name, msg in (("short.bin", "shorter"), ("outside.bin", "particle 20 ")):
            with pytest.raises(pkg.EkpnpError) as e:
                b.tracers_load(str(tmp_path / name))
            assert msg in str(e.value)
        _assert_cloud(b.tracers_get(), want, "a refused load leaves the cloud alone")
    with pkg.Solver(_params(pkg, O)) as o:
        with pytest.raises(pkg.EkpnpError) as e:
            o.tracers_load(path)
        assert "70 x 66 x 13" in str(e.value) and o.tracers_size == 0


# ---- 7. the run is left alone ------------------------------------------------------------------------------------------

def test_advancing_and_recording_leave_the_step_graph_and_the_run_alone(pkg):
    p = _params(pkg, R)
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        _seeded_start(pkg, a)
        _seeded_start(pkg, b)
        a.step(5)
        b.step(5)
        state = a.graph_state()
        assert state == 1
        bytes_before = a.device_bytes()
        a.tracers_seed(n=1000, seed=1)
        assert a.device_bytes() >= bytes_before + 1000 * 56
        a.tracers_arm(capacity=8)
        assert a.graph_state() == state
        for k in range(6):
            a.step(1)
            a.tracers_advance(p.dt, nsub=2, mu=1e-8 if k % 2 else 0.0)
            a.tracers_record(6 + k, a.t)
        b.step(6)
        assert a.graph_state() == state and b.graph_state() == state and a.tracers_count() == (6, 0)
        fa, fb = a.fields(), b.fields()
        for n in pkg.FIELDS:
            assert np.array_equal(T.bits(fa[n]), T.bits(fb[n])), n
        assert b.device_bytes() == bytes_before   # a context that never calls the new entry points allocates nothing new
        a.tracers_release()
        assert a.device_bytes() == bytes_before   # and release gives everything back


def test_slab_contexts_are_refused(pkg):
    p = _params(pkg, W)
    msg = "tracers: slab contexts are not supported"
    x = np.array([1.0])
    for rank, nranks in ((0, 1), (1, 3)):
        with pkg.Solver(p, rank=rank, nranks=nranks, slab=True) as s:
            calls = [lambda: s.tracers_seed(n=10, seed=1), lambda: s.tracers_set(x, x, x), lambda: s.tracers_get(), lambda: s.tracers_size,
                     lambda: s.tracers_release(), lambda: s.tracers_advance(1e-9), lambda: s.tracers_save("unused.bin"), lambda: s.tracers_load("unused.bin"),
                     lambda: s.tracers_cell_counts((1, 1, 1)), lambda: s.tracers_moments(), lambda: s.tracers_arm(4), lambda: s.tracers_disarm(),
                     lambda: s.tracers_record(1, 0.0), lambda: s.tracers_count(), lambda: s.tracers_read(0, 0), lambda: s.tracers_ring_save("unused.dat")]
            for k, call in enumerate(calls):
                with pytest.raises(pkg.EkpnpError) as e:
                    call()
                assert "status 1" in str(e.value) and msg in str(e.value), k
    assert not os.path.exists("unused.bin") and not os.path.exists("unused.dat")


# ---- 8. the driver -----------------------------------------------------------------------------------------------------

def _run_driver(args, out, code=0):
    out.mkdir()
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1", EKPNP_PLACEMENT_TRIES="1")  # the child shares device 0 with this process
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == code, (args, r.stderr[-2000:])
    return out, r.stderr


GEO = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "6", "--seed-pattern", "squares", "--seed-modes", "1,1"]


def test_driver_writes_the_rows_and_the_final_file_of_the_library_calls(pkg, tmp_path):
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
        s.tracers_arm(3)
        t = 0.0
        for i in range(6):
            s.stream_collide_save(t)
            s.fast_Poisson()
            t = t + p.dt
            if (i + 1) % 2 == 0:
                s.tracers_advance(2.0 * p.dt, nsub=3, mu=mu)
                s.tracers_record(i + 1, t)
        s.tracers_ring_save(str(tmp_path / "lib_tracers.dat"))
        s.tracers_save(str(tmp_path / "lib_final.bin"), time=t)
        counts, lost = s.tracers_cell_counts((4, 3, 2))
    flags = ["--tracers", "1000", "--tracers-seed", "9", "--tracers-every", "2", "--tracers-substeps", "3", "--tracers-mobility", "1e-9", "--tracers-cells", "4,3,2"]
    plain, _ = _run_driver(GEO, tmp_path / "plain")
    loop, _ = _run_driver([*GEO, *flags], tmp_path / "loop")
    batch, _ = _run_driver([*GEO, *flags, "--batch", "1"], tmp_path / "batch")
    assert (loop / "tracers.dat").read_bytes() == (tmp_path / "lib_tracers.dat").read_bytes()
    assert (loop / "tracers_final.bin").read_bytes() == (tmp_path / "lib_final.bin").read_bytes()
    lines = (loop / "tracers.dat").read_text().splitlines()
    assert lines[0] == "# ekpnp tracers nx 40 ny 12 nz 17 n 1000 recorded 3 dropped 0" and [ln.split()[0] for ln in lines[2:]] == ["2", "4", "6"]
    cells = (loop / "tracer_cells.dat").read_text().splitlines()
    assert cells[0].startswith("# ekpnp tracer cells nx 40 ny 12 nz 17 bx 4 by 3 bz 2 n 1000 lost %d time " % lost)
    assert np.array_equal(np.array([[int(v) for v in ln.split(" ")] for ln in cells[1:]]).reshape(2, 3, 4), counts)
    for f in ("tracers.dat", "tracers_final.bin", "tracer_cells.dat"):
        assert (loop / f).read_bytes() == (batch / f).read_bytes(), f
        assert not (plain / f).exists()
    for f in ("data.dat", "umax.dat", "data_end.dat"):
        x = (plain / f).read_bytes()
        assert len(x) > 0 and x == (loop / f).read_bytes() and x == (batch / f).read_bytes(), f
    assert sorted(os.listdir(loop)) == sorted(os.listdir(plain) + ["tracers.dat", "tracers_final.bin", "tracer_cells.dat"])
    # a grid over the default box, no cells
    grid, _ = _run_driver([*GEO, "--tracers-grid", "8,4,5"], tmp_path / "grid")
    raw = (grid / "tracers_final.bin").read_bytes()
    assert len(raw) == 48 + 160 * 56 and not (grid / "tracer_cells.dat").exists()
    gx, gy, gz = pkg.tracers_seed_host(p, pkg.tracers_spec(grid=(8, 4, 5), p=p))
    start = np.frombuffer(raw[48 + 3 * 160 * 8:48 + 6 * 160 * 8], dtype="<f8").reshape(3, 160)
    assert T.same(start[0], gx) and T.same(start[1], gy) and T.same(start[2], gz)
    assert len((grid / "tracers.dat").read_text().splitlines()) == 2 + 6   # --tracers-every defaults to 1
    for bad, number in ((["--tracers", "0"], "n = 0"), (["--tracers", "12x"], "got 12x"), (["--tracers-grid", "4,4"], "got 4,4"),
                        (["--tracers", "10", "--tracers-box", "0,41,0,12,1,15"], "hi = 41"), (["--tracers", "10", "--tracers-box", "0,40,0,12"], "got 0,40,0,12"),
                        (["--tracers", "10", "--tracers-every", "0"], "got 0"), (["--tracers", "10", "--tracers-substeps", "5000"], "got 5000"),
                        (["--tracers", "10", "--tracers-mobility", "fast"], "got fast"), (["--tracers", "10", "--tracers-cells", "41,1,1"], "bx = 41"),
                        (["--tracers", "10", "--gpus", "2", "--devices", "0,0"], "slab contexts are not supported")):
        _, err = _run_driver([*GEO, *bad], tmp_path / ("bad" + "_".join(bad).replace("-", "").replace(",", "_")), code=2)
        assert number in err, err
