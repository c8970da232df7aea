"""The definition of a tracer advance (include/ekpnp.h, the tracers block) transcribed into numpy, operation by operation, and the
inputs the CPU and the GPU tests of the tracers share.  numpy rounds every ufunc once and fuses nothing, so the transcription and
ekpnp_tracers_advance_host must agree on the float64 BIT PATTERN."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def _lerp(p, q, f):
    d = q - p
    t = f * d
    return p + t


def _stencil(dims, x, y, z):
    nx, ny, nz = dims
    i0 = x.astype(np.int64)
    fx = x - i0.astype(np.float64)
    i1 = np.where(i0 + 1 == nx, 0, i0 + 1)
    j0 = y.astype(np.int64)
    fy = y - j0.astype(np.float64)
    j1 = np.where(j0 + 1 == ny, 0, j0 + 1)
    k0 = np.minimum(z.astype(np.int64), nz - 2)
    fz = z - k0.astype(np.float64)
    return i0, i1, fx, j0, j1, fy, k0, k0 + 1, fz


def _value(a, st):
    i0, i1, fx, j0, j1, fy, k0, k1, fz = st
    a00 = _lerp(a[k0, j0, i0], a[k0, j0, i1], fx)
    a10 = _lerp(a[k0, j1, i0], a[k0, j1, i1], fx)
    a01 = _lerp(a[k1, j0, i0], a[k1, j0, i1], fx)
    a11 = _lerp(a[k1, j1, i0], a[k1, j1, i1], fx)
    b0 = _lerp(a00, a10, fy)
    b1 = _lerp(a01, a11, fy)
    return _lerp(b0, b1, fz)


def _velocity(dims, u, E, mu, x, y, z):
    st = _stencil(dims, x, y, z)
    w = []
    for c in range(3):
        v = _value(u[c], st)
        if mu != 0.0:
            t = mu * _value(E[c], st)
            v = v + t
        w.append(v)
    return w


def _fold(x, n, w):
    up = x >= n
    dn = ~up & (x < 0.0)
    x = np.where(up, x - n, np.where(dn, x + n, x))
    w = w + up.astype(np.int32) - dn.astype(np.int32)
    up = x >= n
    x = np.where(up, x - n, x)
    w = w + up.astype(np.int32)
    return x, w, (x >= 0.0) & (x < n)


def _fold_z(z, top):
    ok = np.isfinite(z)
    z = np.where(z < 0.0, 0.0, z)
    z = np.where(z > top, top, z)
    return z, ok


def advance(p, u, x, y, z, wx=None, wy=None, E=None, mu=0.0, h=0.0, nsub=1):
    """new (x, y, z, wx, wy): the definition, vectorised over the particles"""
    dims = (p.nx, p.ny, p.nz)
    pnx, pny, top = float(p.nx), float(p.ny), float(p.nz - 1)
    hx, hy, hz = h / p.dx, h / p.dy, h / p.dz
    ax, ay, az = 0.5 * hx, 0.5 * hy, 0.5 * hz
    x, y, z = (np.array(a, dtype=np.float64) for a in (x, y, z))
    wx = np.zeros(x.size, np.int32) if wx is None else np.array(wx, dtype=np.int32)
    wy = np.zeros(x.size, np.int32) if wy is None else np.array(wy, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(nsub):
            a = np.flatnonzero(~(np.isnan(x) | np.isnan(y) | np.isnan(z)))  # the lost ones are skipped
            if a.size == 0:
                break
            xa, ya, za = x[a], y[a], z[a]
            w = _velocity(dims, u, E, mu, xa, ya, za)
            none = np.zeros(a.size, np.int32)
            x1, _, okx = _fold(xa + ax * w[0], pnx, none)
            y1, _, oky = _fold(ya + ay * w[1], pny, none)
            z1, okz = _fold_z(za + az * w[2], top)
            ok = okx & oky & okz
            w = _velocity(dims, u, E, mu, np.where(ok, x1, 0.0), np.where(ok, y1, 0.0), np.where(ok, z1, 0.0))
            x2, wx2, okx = _fold(xa + hx * w[0], pnx, wx[a])
            y2, wy2, oky = _fold(ya + hy * w[1], pny, wy[a])
            z2, okz = _fold_z(za + hz * w[2], top)
            ok = ok & okx & oky & okz
            x[a] = np.where(ok, x2, np.nan)
            y[a] = np.where(ok, y2, np.nan)
            z[a] = np.where(ok, z2, np.nan)
            wx[a] = np.where(ok, wx2, wx[a])  # a lost particle keeps its image counts
            wy[a] = np.where(ok, wy2, wy[a])
    return x, y, z, wx, wy


def cell(dims, cells, x, y, z):
    """the integer definition of ekpnp_tracers_cell, -1 for a lost particle"""
    nx, ny, nz = dims
    bx, by, bz = cells
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    lost = np.isnan(x) | np.isnan(y) | np.isnan(z)
    xs, ys, zs = (np.where(lost, 0.0, a) for a in (x, y, z))
    i0, j0, k0 = xs.astype(np.int64), ys.astype(np.int64), np.minimum(zs.astype(np.int64), nz - 2)
    c = ((k0 * bz) // (nz - 1) * by + (j0 * by) // ny) * bx + (i0 * bx) // nx
    return np.where(lost, -1, c)


def random_fields(shape, seed, u_scale=1e-3, e_scale=1e5):
    """(u, E): three velocity and three field arrays [nz, ny, nx]"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    u = [u_scale * rng.uniform(-1.0, 1.0, size=(nz, ny, nx)) for _ in range(3)]
    E = [e_scale * rng.uniform(-1.0, 1.0, size=(nz, ny, nx)) for _ in range(3)]
    return u, E


U_SCALE, E_SCALE, MU = 1e-3, 1e5, 1e-8   # mu*E is of the size of u


def substep(p, cells=3.0):
    """h such that the fastest node moves a particle about `cells` cells per substep along x"""
    return cells * p.dx / U_SCALE


def special_cloud(shape, n, seed):
    """n positions: random ones, and in front of them the special ones of the issue (where n allows)"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, nx, n)
    y = rng.uniform(0.0, ny, n)
    z = rng.uniform(0.0, nz - 1, n)
    x[x >= nx] = 0.0
    y[y >= ny] = 0.0
    special = [
        (nx - 0.25, 1.5, 2.5),                              # the wrap of the stencil along x
        (3.5, np.nextafter(float(ny), 0.0), 2.5),           # y one ulp below ny
        (5.5, 4.5, 0.0),                                    # on the lower plate
        (6.5, 5.5, float(nz - 1)),                          # on the upper plate: fz == 1
        (7.5, 6.5, np.nextafter(float(nz - 1), 0.0)),       # just below it
        (0.125, 7.5, 1.5), (nx - 0.125, 8.5, 1.5),          # about to wrap either way along x ...
        (9.5, 0.125, 1.5), (10.5, ny - 0.125, 1.5),         # ... and along y
        (11.5, 9.5, 0.125), (12.5, 10.5, nz - 1.125),       # about to meet either plate
        (np.nan, np.nan, np.nan),                           # lost from the start
    ]
    for k, (a, b, c) in enumerate(special[:n - 1]):  # particle 0 stays a random one
        x[k + 1], y[k + 1], z[k + 1] = a, b, c
    return x, y, z
