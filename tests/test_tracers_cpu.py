"""CPU tests of the Lagrangian tracers (csrc/tracers.hip; include/ekpnp.h: ekpnp_tracers_*): the host-only entry points, which ARE
the definitions the device is held against in tests/test_tracers_gpu.py.  No device is needed.

ekpnp_tracers_advance_host is compared with a numpy transcription of the header's text (tests/_tracers_ref.py) on the float64 BIT
PATTERN; the exact cases use dyadic numbers, so every product and sum is exact and the expected result is known in closed form."""
import ctypes as C
import math

import numpy as np
import pytest

import _tracers_ref as T

W = (70, 66, 13)

NAMES = [
    "ekpnp_tracers_spec_check", "ekpnp_tracers_seed_host", "ekpnp_tracers_advance_host", "ekpnp_tracers_cell", "ekpnp_tracers_seed",
    "ekpnp_tracers_set", "ekpnp_tracers_get", "ekpnp_tracers_size", "ekpnp_tracers_release", "ekpnp_tracers_advance", "ekpnp_tracers_save",
    "ekpnp_tracers_load", "ekpnp_tracers_cell_counts", "ekpnp_tracers_moments", "ekpnp_tracers_arm", "ekpnp_tracers_disarm",
    "ekpnp_tracers_record", "ekpnp_tracers_count", "ekpnp_tracers_read", "ekpnp_tracers_ring_save",
]
METHODS = ["tracers_seed", "tracers_set", "tracers_get", "tracers_size", "tracers_release", "tracers_advance", "tracers_save", "tracers_load",
           "tracers_cell_counts", "tracers_moments", "tracers_arm", "tracers_disarm", "tracers_record", "tracers_count", "tracers_read",
           "tracers_ring_save"]


def _dyadic_params(pkg, shape):
    """dx = dy = dz = 2^-17 m: with h = 2^-10 s the step constants are hx = hy = hz = 128, ax = 64, exactly"""
    p = pkg.default_params(*shape)
    p.dx = p.dy = p.dz = 2.0 ** -17
    return p


# ---- 1. the interface ------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_mirrored(pkg):
    lib = pkg.load_library()
    for name in NAMES:
        assert name in pkg.exported_symbols()
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    assert not [n for n in pkg.exported_symbols() if n.startswith("ekpnp_group_tracers")]
    assert C.sizeof(pkg.TracersSpec) == 80
    assert [f[0] for f in pkg.TracersSpec._fields_] == ["n", "mode", "gx", "gy", "gz", "seed", "lo", "hi"]
    assert [getattr(pkg.TracersSpec, n).offset for n in ("n", "mode", "gx", "gy", "gz", "seed", "lo", "hi")] == [0, 8, 12, 16, 20, 24, 32, 56]
    for m in METHODS:
        assert hasattr(pkg.Solver, m), m
    assert not [m for m in dir(pkg.Group) if "tracers" in m]
    assert len(pkg.TRACER_MOMENTS) == 12 and pkg.TRACER_MOMENTS[:2] == ["alive", "lost"] and pkg.TRACER_MOMENTS[-2:] == ["z_min", "z_max"]
    assert (pkg.TRACERS_RANDOM, pkg.TRACERS_GRID) == (0, 1)


def _refused(pkg, p, spec):
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.tracers_spec_check(p, spec)
    return str(e.value)


def test_bad_specs_are_refused_with_the_offending_number(pkg):
    p = pkg.default_params(*W)
    good = pkg.tracers_spec(n=100, p=p)
    assert pkg.tracers_spec_check(p, good) is good
    assert pkg.tracers_spec_check(p, pkg.tracers_spec(grid=(5, 4, 3), p=p)).n == 60
    assert pkg.tracers_spec_check(p, pkg.tracers_spec(n=1 << 28, box=((0, 70), (0, 66), (0, 12)))).n == 1 << 28
    assert "n = 0" in _refused(pkg, p, pkg.tracers_spec(n=0, p=p))
    assert "n = 268435457" in _refused(pkg, p, pkg.tracers_spec(n=(1 << 28) + 1, p=p))
    s = pkg.tracers_spec(n=100, p=p)
    s.mode = 2
    assert "mode = 2" in _refused(pkg, p, s)
    assert "5*4*3" in _refused(pkg, p, pkg.tracers_spec(n=61, grid=(5, 4, 3), p=p))
    assert "gy = 0" in _refused(pkg, p, pkg.tracers_spec(n=15, grid=(5, 0, 3), p=p))
    s = pkg.tracers_spec(n=100, p=p)
    s.gz = 7
    assert "gz = 7" in _refused(pkg, p, s)
    assert "hi = 70.5" in _refused(pkg, p, pkg.tracers_spec(n=10, box=((0, 70.5), (0, 66), (1, 11))))
    assert "lo = -0.5" in _refused(pkg, p, pkg.tracers_spec(n=10, box=((0, 70), (-0.5, 66), (1, 11))))
    assert "hi = 12.25" in _refused(pkg, p, pkg.tracers_spec(n=10, box=((0, 70), (0, 66), (1, 12.25))))
    assert "hi = 3" in _refused(pkg, p, pkg.tracers_spec(n=10, box=((3, 3), (0, 66), (1, 11))))
    assert "nan" in _refused(pkg, p, pkg.tracers_spec(n=10, box=((0, 70), (0, math.nan), (1, 11)))).lower()
    assert "inf" in _refused(pkg, p, pkg.tracers_spec(n=10, box=((0, math.inf), (0, 66), (1, 11)))).lower()
    thin = pkg.default_params(8, 8, 8)
    thin.nz = 2
    assert "nz = 2" in _refused(pkg, thin, pkg.tracers_spec(n=10, box=((0, 8), (0, 8), (0, 1))))


def test_null_pointers_are_refused_not_dereferenced(pkg):
    L = pkg.load_library()
    p = pkg.default_params(*W)
    spec = pkg.tracers_spec(n=10, p=p)
    a = np.zeros(10)
    w = np.zeros(10, dtype=np.int32)
    u = np.zeros((W[2], W[1], W[0]))
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    assert L.ekpnp_tracers_spec_check(None, C.byref(spec)) == 1 and b"NULL" in L.ekpnp_last_error(None)
    assert L.ekpnp_tracers_spec_check(C.byref(p), None) == 1 and b"NULL" in L.ekpnp_last_error(None)
    assert L.ekpnp_tracers_seed_host(C.byref(p), C.byref(spec), 0, 10, ptr(a), None, ptr(a)) == 1 and b"NULL" in L.ekpnp_last_error(None)
    assert L.ekpnp_tracers_seed_host(C.byref(p), C.byref(spec), 5, 6, ptr(a), ptr(a), ptr(a)) == 1 and b"n = 10" in L.ekpnp_last_error(None)
    args = [C.byref(p), ptr(u), ptr(u), ptr(u), None, None, None, 0.0, 1e-9, 1, 10, ptr(a), ptr(a), ptr(a), ptr(w), ptr(w)]
    assert L.ekpnp_tracers_advance_host(*args) == 0  # mu == 0: the E arrays are not needed
    args[7] = 1e-8
    assert L.ekpnp_tracers_advance_host(*args) == 1 and b"NULL" in L.ekpnp_last_error(None)
    args[7] = 0.0
    for k in (1, 11, 14):
        bad = list(args)
        bad[k] = None
        assert L.ekpnp_tracers_advance_host(*bad) == 1 and b"NULL" in L.ekpnp_last_error(None)
    for k, v, msg in ((9, 0, b"nsub = 0"), (9, 4097, b"nsub = 4097"), (8, math.inf, b"h = inf"), (10, -1, b"n = -1")):
        bad = list(args)
        bad[k] = v
        assert L.ekpnp_tracers_advance_host(*bad) == 1 and msg in L.ekpnp_last_error(None)
    assert L.ekpnp_tracers_cell(None, 2, 2, 2, 1.0, 1.0, 1.0) == -2
    assert L.ekpnp_tracers_cell(C.byref(p), 71, 2, 2, 1.0, 1.0, 1.0) == -2 and b"bx = 71" in L.ekpnp_last_error(None)
    assert L.ekpnp_tracers_cell(C.byref(p), 64, 64, 12, 1.0, 1.0, 1.0) >= 0
    assert L.ekpnp_tracers_cell(C.byref(p), 64, 66, 12, 1.0, 1.0, 1.0) >= 0
    assert L.ekpnp_tracers_cell(C.byref(p), 70, 66, 12, 1.0, 1.0, 1.0) >= 0
    assert L.ekpnp_tracers_cell(C.byref(p), 70, 66, 13, 1.0, 1.0, 1.0) == -2 and b"bz = 13" in L.ekpnp_last_error(None)
    wide = pkg.default_params(128, 64, 17)
    assert L.ekpnp_tracers_cell(C.byref(wide), 128, 32, 16, 1.0, 1.0, 1.0) >= 0   # 65536 cells
    assert L.ekpnp_tracers_cell(C.byref(wide), 128, 64, 16, 1.0, 1.0, 1.0) == -2 and b"bx*by*bz = 131072" in L.ekpnp_last_error(None)
    for name in ("seed", "release", "disarm"):
        assert getattr(L, "ekpnp_tracers_" + name)(None, *([None] if name == "seed" else [])) == 1


# ---- 2. seeding ------------------------------------------------------------------------------------------------------

def test_grid_seed_equals_the_formula(pkg):
    p = pkg.default_params(*W)
    box = ((0.0, 70.0), (2.5, 60.25), (1.0, 11.0))
    g = (7, 5, 3)
    x, y, z = pkg.tracers_seed_host(p, pkg.tracers_spec(grid=g, box=box))
    assert x.size == 105
    for q in range(105):
        i, j, k = q % 7, (q // 7) % 5, q // 35
        want = [box[a][0] + ((float(idx) + 0.5) * (box[a][1] - box[a][0])) / float(g[a]) for a, idx in enumerate((i, j, k))]
        assert [x[q], y[q], z[q]] == want, q
    # a whole-lattice grid: one particle per node column centre, all inside
    x, y, z = pkg.tracers_seed_host(p, pkg.tracers_spec(grid=(70, 66, 2), box=((0, 70), (0, 66), (0, 12))))
    assert x.min() == 0.5 and x.max() == 69.5 and y.max() == 65.5 and set(z) == {3.0, 9.0}


def test_random_seed_equals_a_transcription_and_lies_in_its_box(pkg):
    p = pkg.default_params(*W)
    L = pkg.load_library()
    for box, seed in ((((0.0, 70.0), (0.0, 66.0), (1.0, 11.0)), 5), (((3.25, 3.5), (65.0, 66.0), (0.0, 12.0)), 2 ** 63 + 11)):
        spec = pkg.tracers_spec(n=1000, box=box, seed=seed)
        x, y, z = pkg.tracers_seed_host(p, spec)
        for a, got in enumerate((x, y, z)):
            lo, hi = box[a]
            r = np.array([L.ekpnp_seed_uniform(seed, q, 16 + a) for q in range(1000)])
            assert r.min() >= -1.0 and r.max() < 1.0
            u = 0.5 * r + 0.5
            v = lo + u * (hi - lo)
            v = np.where(v >= hi, lo, v)
            assert T.same(got, v), a
            assert got.min() >= lo and got.max() < hi
        assert len(set(x)) > 990  # the axes and the particles draw different numbers
        assert not np.array_equal(x - box[0][0], (y - box[1][0]) * (box[0][1] - box[0][0]) / (box[1][1] - box[1][0]))
    # in pieces: the bits of seeding at once, in both modes
    for spec in (pkg.tracers_spec(n=1000, p=p, seed=9), pkg.tracers_spec(grid=(10, 10, 10), p=p)):
        whole = pkg.tracers_seed_host(p, spec)
        pieces = [pkg.tracers_seed_host(p, spec, first, count) for first, count in ((0, 1), (1, 255), (256, 0), (256, 744))]
        for a in range(3):
            assert T.same(np.concatenate([q[a] for q in pieces]), whole[a])


# ---- 3. the advance against its transcription --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def w_case(pkg):
    p = pkg.default_params(*W)
    u, E = T.random_fields(W, 71, T.U_SCALE, T.E_SCALE)
    x, y, z = T.special_cloud(W, 1000, 72)
    for a in (*u, *E, x, y, z):
        a.setflags(write=False)
    return p, u, E, x, y, z


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("mu", [0.0, T.MU])
def test_advance_host_equals_the_transcription_bit_for_bit(pkg, w_case, mu, sign):
    p, u, E, x, y, z = w_case
    h = sign * T.substep(p)
    got = pkg.tracers_advance_host(p, u, x, y, z, E=E, mu=mu, h=h, nsub=7)
    want = T.advance(p, u, x, y, z, E=E, mu=mu, h=h, nsub=7)
    for k, name in enumerate(("x", "y", "z")):
        assert T.same(got[k], want[k]), (name, np.flatnonzero(T.bits(got[k]) != T.bits(want[k]))[:5])
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    gx, gy, gz, wx, wy = got
    lost = np.isnan(gx)
    assert np.array_equal(lost, np.isnan(gy)) and np.array_equal(lost, np.isnan(gz))
    assert lost[12] and lost.sum() == 1  # the particle lost from the start, and nobody else at three cells per substep
    alive = ~lost
    assert (gx[alive] >= 0).all() and (gx[alive] < W[0]).all() and (gy[alive] >= 0).all() and (gy[alive] < W[1]).all()
    assert (gz[alive] >= 0).all() and (gz[alive] <= W[2] - 1).all()
    # the cases the issue names did happen: wraps either way along both axes, and particles held by either plate
    assert (wx > 0).any() and (wx < 0).any() and (wy > 0).any() and (wy < 0).any()
    assert (gz[alive] == 0.0).any() and (gz[alive] == W[2] - 1).any()
    # the velocity really moved them by cells, and mu matters
    assert np.abs(gx[alive] + wx[alive] * W[0] - x[alive]).max() > 3.0
    if mu != 0.0:
        passive = pkg.tracers_advance_host(p, u, x, y, z, mu=0.0, h=h, nsub=7)
        assert not T.same(passive[0], gx)


def test_advance_in_one_call_equals_substep_by_substep(pkg, w_case):
    p, u, E, x, y, z = w_case
    h = T.substep(p)
    whole = pkg.tracers_advance_host(p, u, x, y, z, E=E, mu=T.MU, h=h, nsub=7)
    s = (x, y, z, None, None)
    for _ in range(7):
        s = pkg.tracers_advance_host(p, u, *s, E=E, mu=T.MU, h=h, nsub=1)
    for k in range(3):
        assert T.same(whole[k], s[k])
    assert np.array_equal(whole[3], s[3]) and np.array_equal(whole[4], s[4])


# ---- 4. exact cases ----------------------------------------------------------------------------------------------------

def test_uniform_velocity_moves_three_cells_exactly_and_counts_the_wraps(pkg):
    p = _dyadic_params(pkg, W)
    nz, ny, nx = W[2], W[1], W[0]
    h = 2.0 ** -10                      # hx = 128
    u = [np.full((nz, ny, nx), 0.375 / 128.0), np.full((nz, ny, nx), -0.375 / 128.0), np.zeros((nz, ny, nx))]
    x0 = np.array([10.25, nx - 1.5, 0.5, nx - 3.0])
    y0 = np.array([20.5, 1.5, ny - 0.5, 3.0])
    z0 = np.array([3.0, 0.0, 12.0, 6.5])
    x, y, z, wx, wy = pkg.tracers_advance_host(p, u, x0, y0, z0, h=h, nsub=8)
    assert x.tolist() == [13.25, 1.5, 3.5, 0.0] and wx.tolist() == [0, 1, 0, 1]
    assert y.tolist() == [17.5, ny - 1.5, ny - 3.5, 0.0] and wy.tolist() == [0, -1, 0, 0]
    assert z.tolist() == z0.tolist()
    xb, yb, zb, wxb, wyb = pkg.tracers_advance_host(p, u, x, y, z, wx, wy, h=-h, nsub=8)  # and back
    assert xb.tolist() == x0.tolist() and yb.tolist() == y0.tolist() and wxb.tolist() == [0, 0, 0, 0] and wyb.tolist() == [0, 0, 0, 0]


def test_a_linear_profile_is_interpolated_exactly(pkg):
    p = _dyadic_params(pkg, W)
    nz, ny, nx = W[2], W[1], W[0]
    a = 2.0 ** -10
    zz = np.arange(nz, dtype=np.float64)[:, None, None]
    u = [np.broadcast_to(a * zz, (nz, ny, nx)).copy(), np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx))]
    z0 = np.array([0.0, 2.5, 7.25, 11.75, 12.0])
    x0 = np.full(5, 1.0)
    y0 = np.array([0.0, 13.5, 65.5, 7.0, 30.25])
    x, y, z, wx, wy = pkg.tracers_advance_host(p, u, x0, y0, z0, h=2.0 ** -10, nsub=4)
    assert x.tolist() == (1.0 + 4 * 128.0 * a * z0).tolist()  # ux = a z at any z: 4 substeps of hx a z
    assert y.tolist() == y0.tolist() and z.tolist() == z0.tolist() and not wx.any() and not wy.any()


def test_a_nan_node_loses_exactly_the_particles_whose_stencil_holds_it(pkg):
    p = pkg.default_params(*W)
    nz, ny, nx = W[2], W[1], W[0]
    for node in ((5, 7, 9), (0, 0, 0), (nz - 1, ny - 1, nx - 1)):
        u = [np.zeros((nz, ny, nx)) for _ in range(3)]
        u[1][node] = np.nan
        kk, jj, ii = np.meshgrid(np.arange(nz - 1), np.arange(ny), np.arange(nx), indexing="ij")
        x0, y0, z0 = ii.ravel() + 0.5, jj.ravel() + 0.25, kk.ravel() + 0.75
        x, y, z, wx, wy = pkg.tracers_advance_host(p, u, x0, y0, z0, h=1e-9, nsub=2)
        k, j, i = node
        holds = np.isin(kk.ravel(), [k - 1, k]) & np.isin(jj.ravel(), [(j - 1) % ny, j]) & np.isin(ii.ravel(), [(i - 1) % nx, i])
        assert holds.sum() == (8 if 0 < k < nz - 1 else 4)
        lost = np.isnan(x)
        assert np.array_equal(lost, holds) and np.array_equal(np.isnan(y), holds) and np.array_equal(np.isnan(z), holds)
        assert T.same(x[~lost], x0[~lost]) and T.same(y[~lost], y0[~lost]) and T.same(z[~lost], z0[~lost])  # nobody else moved
        assert not wx.any() and not wy.any()
    # an infinite node does the same, and in the E arrays only when mu != 0
    u = [np.zeros((nz, ny, nx)) for _ in range(3)]
    E = [np.zeros((nz, ny, nx)) for _ in range(3)]
    E[2][5, 7, 9] = np.inf
    x, y, z, _, _ = pkg.tracers_advance_host(p, u, [8.5, 20.5], [6.5, 6.5], [4.5, 4.5], E=E, mu=0.0, h=1e-9)
    assert not np.isnan(x).any()
    x, y, z, _, _ = pkg.tracers_advance_host(p, u, [8.5, 20.5], [6.5, 6.5], [4.5, 4.5], E=E, mu=1e-8, h=1e-9)
    assert np.isnan(x).tolist() == [True, False] and np.isnan(z).tolist() == [True, False]


def test_a_displacement_beyond_one_period_loses_the_particle(pkg):
    p = _dyadic_params(pkg, (64, 32, 9))
    nz, ny, nx = 9, 32, 64
    h = 2.0 ** -10                      # hx = 128

    def run(periods, axis, x0=16.0, y0=8.0, wx=(3,), wy=(-2,)):
        u = [np.zeros((nz, ny, nx)) for _ in range(3)]
        u[axis][...] = periods * (nx if axis == 0 else ny) / 128.0
        return pkg.tracers_advance_host(p, u, [x0], [y0], [4.0], wx, wy, h=h, nsub=1)

    x, y, z, wx, wy = run(0.5, 0)
    assert (x[0], y[0], z[0], wx[0], wy[0]) == (48.0, 8.0, 4.0, 3, -2)
    x, y, z, wx, wy = run(1.0, 0)        # one whole period: the same place, one image further
    assert (x[0], wx[0]) == (16.0, 4)
    for periods, axis in ((-1.5, 0), (4.0, 0), (-1.5, 1), (4.0, 1)):
        x, y, z, wx, wy = run(periods, axis)
        assert np.isnan(x[0]) and np.isnan(y[0]) and np.isnan(z[0]), (periods, axis)
        assert (wx[0], wy[0]) == (3, -2)  # the image counts stay what they were


# ---- 5. the order of the scheme ------------------------------------------------------------------------------------------

def test_the_midpoint_scheme_is_second_order(pkg):
    """dz/dt = -(z - 6) in lattice units (uz = -(z - 6) dz m/s), z(0) = 9: z(1) = 6 + 3/e.  The midpoint rule multiplies z - 6 by
    1 - h + h^2/2 per substep; that scalar recurrence gives error ratios 4.20 and 4.10, second order gives 4."""
    nx, ny, nz = 8, 8, 13
    p = pkg.default_params(nx, ny, nz)
    zz = np.arange(nz, dtype=np.float64)[:, None, None]
    u = [np.zeros((nz, ny, nx)), np.zeros((nz, ny, nx)), np.broadcast_to(-(zz - 6.0) * p.dz, (nz, ny, nx)).copy()]
    exact = 6.0 + 3.0 * math.exp(-1.0)
    err = []
    for m in (8, 16, 32):
        x, y, z, _, _ = pkg.tracers_advance_host(p, u, [3.5], [2.25], [9.0], h=1.0 / m, nsub=m)
        assert (x[0], y[0]) == (3.5, 2.25)
        err.append(abs(z[0] - exact))
    r1, r2 = err[0] / err[1], err[1] / err[2]
    print(f"errors {err}, ratios {r1:.3f} {r2:.3f}")
    assert 3.5 <= r1 <= 4.5 and 3.5 <= r2 <= 4.5, (err, r1, r2)


# ---- 6. cells ----------------------------------------------------------------------------------------------------------

def test_the_cell_function_equals_its_integer_definition(pkg):
    p = pkg.default_params(*W)
    x, y, z = T.special_cloud(W, 1000, 73)
    for cells in ((1, 1, 1), (4, 3, 2), (70, 66, 12), (7, 11, 5), (64, 32, 12)):
        got = pkg.tracers_cell(p, cells, x, y, z)
        want = T.cell(W, cells, x, y, z)
        assert np.array_equal(got, want), cells
        assert got[12] == -1 and (got >= 0).sum() == 999 and got.max() < cells[0] * cells[1] * cells[2]
    # the upper plate belongs to the last layer of cells
    assert pkg.tracers_cell(p, (1, 1, 12), [0.0], [0.0], [12.0])[0] == 11
    assert pkg.tracers_cell(p, (70, 66, 1), [69.999], [65.999], [0.0])[0] == 70 * 66 - 1
