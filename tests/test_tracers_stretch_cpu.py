"""CPU tests of the flow-map gradient of the tracers (csrc/tracers.hip; include/ekpnp.h: ekpnp_tracers_advance_tangent_host,
ekpnp_stretch_level): the host-only entry points, which ARE the definitions the device is held against in
tests/test_tracers_stretch_gpu.py.  No device is needed.  Every test here fails on the parent commit: the symbols do not exist there.

The advance is compared with a numpy transcription of the header's text (tests/_tracers_stretch_ref.py) on the float64 BIT PATTERN
of F, on e, and on the five cloud arrays, which are also those of ekpnp_tracers_advance_host.  The analytic cases (zero field, shear,
stagnation point) and the finite-difference check have the bounds the rounding of their own arithmetic gives."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _tracers_ref as T
import _tracers_stretch_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ekpnp_tracers_advance_tangent_host", "ekpnp_stretch_level", "ekpnp_tracers_stretch_begin", "ekpnp_tracers_stretch_end", "ekpnp_tracers_advance_tangent",
         "ekpnp_tracers_stretch_get", "ekpnp_tracers_stretch_levels", "ekpnp_tracers_stretch_save", "ekpnp_tracers_stretch_load"]
N = 4097
NSUBS = (1, 7, 100)


# ---- 8. the interface ------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_mirrored(pkg):
    lib = pkg.load_library()
    for name in NAMES:
        assert name in pkg.exported_symbols()
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    assert not [n for n in pkg.exported_symbols() if n.startswith("ekpnp_group_tracers") or n.startswith("ekpnp_group_stretch")]
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ekpnp.h")).read())
    for decl in ("double mu, double h, int nsub, int64_t n, double* x, double* y, double* z, int32_t* wx, int32_t* wy, double* F /* [9][n] */, int32_t* e);",
                 "int32_t ekpnp_stretch_level(const double F[9], int32_t e);",
                 "int ekpnp_tracers_stretch_begin(ekpnp_ctx* ctx);", "int ekpnp_tracers_stretch_end(ekpnp_ctx* ctx);",
                 "int ekpnp_tracers_advance_tangent(ekpnp_ctx* ctx, double mu, double h, int nsub);",
                 "int ekpnp_tracers_stretch_get(ekpnp_ctx* ctx, double* F /* [9][n] */, int32_t* e);",
                 "int ekpnp_tracers_stretch_levels(ekpnp_ctx* ctx, int l_lo, int nlevels, int64_t* counts /* [nlevels+2] */, int64_t* none);",
                 "int ekpnp_tracers_stretch_save(ekpnp_ctx* ctx, const char* path);", "int ekpnp_tracers_stretch_load(ekpnp_ctx* ctx, const char* path);"):
        assert decl in hdr, decl
    hdr = re.sub(r"\s+", " ", re.sub(r"\n \*", " ", open(os.path.join(ROOT, "include", "ekpnp.h")).read()))   # a comment's line starts dropped
    for said in ("EVERY SUM OF THREE TERMS IS ADDED AS (t0 + t1) + t2", "THE PLATE HOLD (the z clamp of step 6) IS IGNORED IN J", "F THEN COVERS THE TANGENT ADVANCES ONLY"):
        assert said in hdr, said
    assert len(lib.ekpnp_tracers_advance_tangent_host.argtypes) == 18 and len(lib.ekpnp_tracers_advance_tangent.argtypes) == 4
    for m in ("tracers_stretch_begin", "tracers_stretch_end", "tracers_stretch_get", "tracers_stretch_levels", "tracers_stretch_save", "tracers_stretch_load", "tracers_ftle"):
        assert hasattr(pkg.Solver, m), m
    for f in ("tracers_advance_tangent_host", "stretch_level"):
        assert callable(getattr(pkg, f)), f
    assert not [m for m in dir(pkg.Group) if "tracers" in m or "stretch" in m]
    assert pkg.STRETCH_NO_LEVEL == -2 ** 31
    # the advances before this one kept their signatures
    assert len(lib.ekpnp_tracers_advance_host.argtypes) == 16 and len(lib.ekpnp_tracers_advance.argtypes) == 4 and len(lib.ekpnp_tracers_advance_absorbing.argtypes) == 7


def test_refusals_of_the_host_function_and_null_arguments(pkg):
    lib = pkg.load_library()
    p = pkg.default_params(*S.SHAPES["O"])
    u, E = T.random_fields(S.SHAPES["O"], 3)
    x, y, z = (np.array([1.5]), np.array([2.5]), np.array([1.25]))
    for kw, number in ((dict(nsub=0), "nsub = 0"), (dict(nsub=4097), "nsub = 4097"), (dict(h=float("inf")), "h = inf"), (dict(h=float("nan")), "h = nan"),
                       (dict(mu=float("inf")), "mu = inf"), (dict(mu=1e-8), "NULL pointer")):   # a mobility without the E arrays
        with pytest.raises(pkg.EkpnpError) as e:
            pkg.tracers_advance_tangent_host(p, u, x, y, z, **{"h": 1e-9, **kw})
        assert number in str(e.value) and "status 1" in str(e.value), kw
    with pytest.raises(ValueError):
        pkg.tracers_advance_tangent_host(p, u, x, y, z, F=np.zeros((3, 3, 2)), h=1e-9)
    q = pkg.default_params(8, 8, 8)
    q.nz = 2
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.tracers_advance_tangent_host(q, [np.zeros((2, 8, 8))] * 3, x, y, np.array([0.5]), h=1e-9)
    assert "nz = 2" in str(e.value)
    # the C entry points themselves: NULL parameters, a NULL F, a negative n - each refused with a message, nothing is touched
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    w = np.zeros(1, np.int32)
    F, lev = pkg.stretch_identity(x, y, z)
    args = [ptr(a) for a in u] + [None] * 3 + [0.0, 1e-9, 1, 1, ptr(x), ptr(y), ptr(z), ptr(w), ptr(w), ptr(F), ptr(lev)]
    assert lib.ekpnp_tracers_advance_tangent_host(None, *args) == 1 and b"NULL parameters" in lib.ekpnp_last_error(None)
    for k in (15, 16):
        bad = list(args)
        bad[k] = None
        assert lib.ekpnp_tracers_advance_tangent_host(C.byref(p), *bad) == 1 and b"NULL pointer" in lib.ekpnp_last_error(None)
    bad = list(args)
    bad[9] = -1
    assert lib.ekpnp_tracers_advance_tangent_host(C.byref(p), *bad) == 1 and b"n = -1" in lib.ekpnp_last_error(None)
    assert lib.ekpnp_tracers_advance_tangent_host(C.byref(p), *args) == 0
    assert lib.ekpnp_stretch_level(None, 0) == -2 ** 31
    for name in NAMES[2:]:   # a NULL context is an error of every context call, not a crash
        fn = getattr(lib, name)
        assert fn(None, *[0 if t in (C.c_int32, C.c_int, C.c_double) else None for t in fn.argtypes[1:]]) == 1, name


# ---- 1. - 3. the advance against its transcription ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases(pkg):
    """per lattice: the parameters, random fields and the special cloud of N positions (one lost from the start); made once, never
    modified"""
    out = {}
    for k, shape in S.SHAPES.items():
        p = pkg.default_params(*shape)
        u, E = T.random_fields(shape, 571 + len(out), T.U_SCALE, T.E_SCALE)
        x, y, z = T.special_cloud(shape, N, 581 + len(out))
        for a in (*u, *E, x, y, z):
            a.setflags(write=False)
        out[k] = (p, u, E, x, y, z)
    return out


def _assert_same(got, want, what):
    for k, name in enumerate(("x", "y", "z")):
        assert T.same(got[k], want[k]), (what, name, np.flatnonzero(T.bits(got[k]) != T.bits(want[k]))[:5])
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]), what
    if len(want) > 5:
        assert got[5].shape == (3, 3, got[0].size) and got[6].dtype == np.int32, what
        assert T.same(got[5], want[5]), (what, "F", np.argwhere(T.bits(got[5]) != T.bits(want[5]))[:5])
        assert np.array_equal(got[6], want[6]), (what, "e", np.flatnonzero(got[6] != want[6])[:5])


@pytest.mark.parametrize("shape", ["W", "O", "R", "T"])
def test_advance_tangent_host_equals_the_transcription_bit_for_bit_and_moves_the_cloud_like_the_plain_advance(pkg, cases, shape):
    p, u, E, x, y, z = cases[shape]
    h = T.substep(p)
    top = float(p.nz - 1)
    seen = {}
    for mu in (0.0, T.MU):
        for nsub in NSUBS:
            kw = dict(E=E, mu=mu, h=h, nsub=nsub)
            got = pkg.tracers_advance_tangent_host(p, u, x, y, z, **kw)
            want = S.advance(p, u, x, y, z, events=seen, **kw)
            _assert_same(got, want, (shape, mu, nsub))
            _assert_same(got[:5], pkg.tracers_advance_host(p, u, x, y, z, **kw), (shape, mu, nsub, "the plain advance"))   # 2. positions unchanged
            lost = np.isnan(got[0])
            assert lost[12] and np.isnan(got[5][:, :, lost]).all() and not np.isnan(got[5][:, :, ~lost]).any() and (got[6][12] == 0)
            if nsub == 100:
                e = got[6][~lost]
                assert (e > 0).sum() > 100, (shape, mu, (e > 0).sum())
                m = np.abs(got[5][:, :, ~lost]).reshape(9, -1).max(axis=0)
                assert ((m >= 2.0 ** -64) & (m < 2.0 ** 64)).all()
            if nsub == 7:
                assert (got[3] > 0).any() and (got[3] < 0).any() and (got[4] > 0).any() and (got[4] < 0).any()   # wraps both ways
                assert (got[2] == 0.0).any() and (got[2] == top).any()                                              # held at both plates
    assert seen["up"] > 1000 and seen["held0"] > 10 and seen["held1"] > 10, seen
    if shape == "W":
        assert seen["down"] > 0, seen   # the renormalisation did go both ways (a compressible field squeezes some parcels flat)
        got = pkg.tracers_advance_tangent_host(p, u, x, y, z, E=E, mu=0.0, h=h, nsub=100)
        assert (got[6] < 0).any()


def test_two_calls_equal_one(pkg, cases):
    p, u, E, x, y, z = cases["T"]
    h = T.substep(p)
    for mu in (0.0, T.MU):
        a = pkg.tracers_advance_tangent_host(p, u, x, y, z, E=E, mu=mu, h=h, nsub=3)
        b = pkg.tracers_advance_tangent_host(p, u, a[0], a[1], a[2], F=a[5], e=a[6], E=E, mu=mu, h=h, nsub=4, wx=a[3], wy=a[4])
        _assert_same(b, pkg.tracers_advance_tangent_host(p, u, x, y, z, E=E, mu=mu, h=h, nsub=7), ("3 + 4", mu))
    # forty substeps in two calls cross the first renormalisation: e travels with F
    a = pkg.tracers_advance_tangent_host(p, u, x, y, z, h=h, nsub=45)
    b = pkg.tracers_advance_tangent_host(p, u, a[0], a[1], a[2], F=a[5], e=a[6], h=h, nsub=55, wx=a[3], wy=a[4])
    assert (a[6] > 0).any()
    _assert_same(b, pkg.tracers_advance_tangent_host(p, u, x, y, z, h=h, nsub=100), "45 + 55")


# ---- 4. zero and shear fields ------------------------------------------------------------------------------------------

def test_a_zero_field_leaves_the_identity_and_a_shear_fills_one_entry(pkg):
    shape = S.SHAPES["W"]
    nx, ny, nz = shape
    p = pkg.default_params(*shape)
    rng = np.random.default_rng(5)
    n = 500
    x, y, z = rng.uniform(0, nx, n), rng.uniform(0, ny, n), rng.uniform(0, nz - 1, n)
    zero = np.zeros((nz, ny, nx))
    ident = pkg.stretch_identity(x, y, z)[0]
    got = pkg.tracers_advance_tangent_host(p, [zero, zero, zero], x, y, z, h=T.substep(p), nsub=9)
    assert np.array_equal(got[5], ident) and not got[6].any() and T.same(got[0], x) and T.same(got[2], z)
    s = 1e-3
    ux = np.broadcast_to((s * np.arange(nz) / (nz - 1))[:, None, None], (nz, ny, nx)).copy()
    nsub, h = 9, T.substep(p, 2.0)
    got = pkg.tracers_advance_tangent_host(p, [ux, zero, zero], x, y, z, h=h, nsub=nsub)
    assert not np.isnan(got[0]).any() and not got[6].any() and (got[3] != 0).any()
    F = got[5].copy()
    f02 = F[0, 2].copy()
    F[0, 2] = 0.0
    assert np.array_equal(F, ident)
    want = nsub * (h / p.dx) * s / (nz - 1)
    assert np.abs(f02 - want).max() <= 1e-13 * want, np.abs(f02 / want - 1).max()


# ---- 5. the stagnation point -------------------------------------------------------------------------------------------

def test_stagnation_point_stretches_exponentially_and_the_exponent_counts_it(pkg):
    nx, ny, nz = 32, 8, 33
    p = pkg.default_params(nx, ny, nz)
    assert p.dx == p.dz
    s = 2.0 ** -17
    h = 0.5 * p.dx / s
    assert (h / p.dx) * s == 0.5
    ux = np.broadcast_to((s * (np.arange(nx) - 16.0))[None, None, :], (nz, ny, nx)).copy()
    uz = np.broadcast_to((-s * (np.arange(nz) - 16.0))[:, None, None], (nz, ny, nx)).copy()
    x, y, z, wx, wy, F, e = pkg.tracers_advance_tangent_host(p, [ux, np.zeros((nz, ny, nx)), uz], [16.0], [3.5], [16.0], h=h, nsub=200)
    assert (x[0], y[0], z[0], wx[0], wy[0]) == (16.0, 3.5, 16.0, 0, 0)
    assert e[0] == 128
    f00, f22 = 1.625 ** 200 * 2.0 ** -128, 0.625 ** 200 * 2.0 ** -128
    assert abs(f00 - 4353.450572376) < 1e-8
    assert abs(F[0, 0, 0] - f00) <= 1e-12 * f00 and abs(F[2, 2, 0] - f22) <= 1e-12 * f22, (F[0, 0, 0] / f00 - 1, F[2, 2, 0] / f22 - 1)
    assert F[1, 1, 0] == 2.0 ** -128
    off = F[:, :, 0].copy()
    off[np.arange(3), np.arange(3)] = 0.0
    assert not off.any()
    assert pkg.stretch_level(F, e) == 2 * 128 + int(np.floor(np.log2(F[0, 0, 0] ** 2 + F[1, 1, 0] ** 2 + F[2, 2, 0] ** 2)))


# ---- 6. F is the derivative of the advance's own map -------------------------------------------------------------------

def test_F_is_the_derivative_of_the_advances_own_map(pkg):
    """central differences of ekpnp_tracers_advance_host at +-2^-20 cells along each axis, unwrapped, against F: 1e-6 of |F|_F for
    every particle (the rounding of the quotient is about eps * 32 / 2^-20 = 7e-9; a wrong term changes F at order 1e-2)"""
    nx, ny, nz = 32, 8, 33
    p = pkg.default_params(nx, ny, nz)
    assert p.dx == p.dy == p.dz
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    kx, kz = 2.0 * np.pi / nx, np.pi / (nz - 1)
    # psi = A sin(kx x) sin(kz z); ux = d psi / dz, uz = - d psi / dx; the larger of the two amplitudes is the peak speed 1e-3
    A = 1e-3 / max(kx, kz)
    ux = A * kz * np.sin(kx * i) * np.cos(kz * k)
    uz = -A * kx * np.cos(kx * i) * np.sin(kz * k)
    uy = 3e-4 * np.sin(kx * i) * np.sin(kz * k)
    u = [ux, uy, uz]
    h, nsub, n = 0.25 * p.dx / 1e-3, 40, 2000
    rng = np.random.default_rng(1)
    x, y, z = rng.uniform(0.0, nx, n), rng.uniform(0.0, ny, n), rng.uniform(1.0, 31.0, n)
    got = pkg.tracers_advance_tangent_host(p, u, x, y, z, h=h, nsub=nsub)
    assert not np.isnan(got[0]).any() and not got[6].any()
    F = got[5]
    d = 2.0 ** -20
    period = (float(nx), float(ny))

    def end(axis, sign):
        s = [x.copy(), y.copy(), z.copy()]
        s[axis] = s[axis] + sign * d
        off = [np.zeros(n), np.zeros(n)]
        for a in range(2):   # a start pushed across the periodic edge is folded, and the end unfolded by as much
            off[a] = np.floor(s[a] / period[a]) * period[a]
            s[a] = s[a] - off[a]
        r = pkg.tracers_advance_host(p, u, *s, h=h, nsub=nsub)
        assert not np.isnan(r[0]).any()
        return [r[0] + period[0] * r[3] + off[0], r[1] + period[1] * r[4] + off[1], r[2]]

    D = np.empty((3, 3, n))
    for r in range(3):
        hi, lo = end(r, 1.0), end(r, -1.0)
        for c in range(3):
            D[c, r] = (hi[c] - lo[c]) / (2.0 * d)
    err = np.sqrt(((D - F) ** 2).sum(axis=(0, 1))) / np.sqrt((F ** 2).sum(axis=(0, 1)))
    print("largest |D - F| / |F|:", err.max(), "particle", err.argmax(), "above 1e-6:", (err > 1e-6).sum())
    assert (err <= 1e-6).all(), (err.max(), np.flatnonzero(err > 1e-6)[:10])


# ---- 7. the level ------------------------------------------------------------------------------------------------------

def test_stretch_level_is_integer_arithmetic_on_the_exponent(pkg):
    rng = np.random.default_rng(11)
    n = 3000
    F = rng.uniform(-1.0, 1.0, (9, n)) * 2.0 ** rng.integers(-80, 80, (1, n)) * 2.0 ** rng.integers(-3, 3, (9, n))
    F[:, :50] = rng.uniform(-1.0, 1.0, (9, 50)) * 2.0 ** rng.integers(-535, -515, (1, 50))   # trC is subnormal
    F[3:, 50:60] = 0.0
    F[1:3, 50:60] = 0.0   # one entry alone
    e = rng.integers(-64 * 30, 64 * 30, n).astype(np.int32)
    trc = F[0] * F[0]
    for q in range(1, 9):
        trc = trc + F[q] * F[q]
    assert (trc[:50] < 2.0 ** -1022).all() and (trc > 0.0).all()
    m, E = np.frexp(trc)
    want = (2 * e.astype(np.int64) + E - 1).astype(np.int32)
    got = pkg.stretch_level(F, e)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert np.array_equal(S.level(F, e), want)
    # F * 2^-64 with e + 64 is the same gradient and has the same level
    assert np.array_equal(pkg.stretch_level(F[:, 60:] * 2.0 ** -64, e[60:] + 64), want[60:])
    assert np.array_equal(pkg.stretch_level(F[:, 60:] * 2.0 ** 64, e[60:] - 64), want[60:])
    # no level: NaN anywhere, or F = 0
    Z = np.zeros(9)
    assert pkg.stretch_level(Z, 5) == pkg.STRETCH_NO_LEVEL == S.NO_LEVEL
    for q in range(9):
        B = np.ones(9)
        B[q] = np.nan
        assert pkg.stretch_level(B, 0) == pkg.STRETCH_NO_LEVEL
    assert pkg.stretch_level(np.eye(3), 0) == 1 and pkg.stretch_level(np.eye(3), 7) == 15 and pkg.stretch_level(np.eye(3).reshape(9), -7) == -13   # |I|^2 = 3
    assert S.level(np.eye(3).reshape(9, 1), [0])[0] == 1
