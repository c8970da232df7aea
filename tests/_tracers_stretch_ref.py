"""The definition of a tangent tracer advance (include/ekpnp.h, THE FLOW-MAP GRADIENT) transcribed into numpy, operation by operation,
on top of the transcription of the deterministic advance (tests/_tracers_ref.py: the stencil, L, the folds): the gradient of the
interpolant, the Jacobian J of a substep, F <- J F, the renormalisation and the level.  numpy rounds every ufunc once and fuses
nothing, so the transcription and ekpnp_tracers_advance_tangent_host must agree on the float64 BIT PATTERN of F, and on e."""
import numpy as np

import _tracers_ref as T

SHAPES = {"W": (70, 66, 13), "O": (35, 33, 5), "R": (40, 12, 17), "T": (70, 66, 17)}
NO_LEVEL = -2 ** 31


def identity(x, y, z):
    """a record just begun: F = I [3, 3, n], e = 0; F = NaN for a lost particle"""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    F = np.zeros((3, 3, x.size))
    for c in range(3):
        F[c, c] = 1.0
    F[:, :, np.isnan(x) | np.isnan(y) | np.isnan(z)] = np.nan
    return F, np.zeros(x.size, np.int32)


def _value_grad(a, st):
    """(v, [gx, gy, gz]): step 3's value and the derivatives per cell of the interpolant from the same eight nodes"""
    i0, i1, fx, j0, j1, fy, k0, k1, fz = st
    n0, n1, n2, n3 = a[k0, j0, i0], a[k0, j0, i1], a[k0, j1, i0], a[k0, j1, i1]
    n4, n5, n6, n7 = a[k1, j0, i0], a[k1, j0, i1], a[k1, j1, i0], a[k1, j1, i1]
    a00, a10 = T._lerp(n0, n1, fx), T._lerp(n2, n3, fx)
    a01, a11 = T._lerp(n4, n5, fx), T._lerp(n6, n7, fx)
    b0, b1 = T._lerp(a00, a10, fy), T._lerp(a01, a11, fy)
    gx = T._lerp(T._lerp(n1 - n0, n3 - n2, fy), T._lerp(n5 - n4, n7 - n6, fy), fz)
    gy = T._lerp(a10 - a00, a11 - a01, fz)
    gz = b1 - b0
    return T._lerp(b0, b1, fz), [gx, gy, gz]


def _velocity_grad(dims, u, E, mu, x, y, z):
    """(w[c], G[c][r]) at (x, y, z)"""
    st = T._stencil(dims, x, y, z)
    w, G = [], []
    for c in range(3):
        v, g = _value_grad(u[c], st)
        if mu != 0.0:
            ve, ge = _value_grad(E[c], st)
            t = mu * ve
            v = v + t
            for r in range(3):
                t = mu * ge[r]
                g[r] = g[r] + t
        w.append(v)
        G.append(g)
    return w, G


def _renormalise(F, e):
    """F [3][3] of arrays and e in place"""
    m = np.zeros_like(F[0][0])
    for c in range(3):
        for r in range(3):
            a = np.where(F[c][r] < 0.0, 0.0 - F[c][r], F[c][r])
            m = np.where(a > m, a, m)
    big = m >= 2.0 ** 64
    small = ~big & (m > 0.0) & (m < 2.0 ** -64)
    for c in range(3):
        for r in range(3):
            F[c][r] = np.where(big, F[c][r] * 2.0 ** -64, np.where(small, F[c][r] * 2.0 ** 64, F[c][r]))
    return F, e + np.where(big, 64, 0).astype(np.int32) - np.where(small, 64, 0).astype(np.int32)


def advance(p, u, x, y, z, F=None, e=None, E=None, mu=0.0, h=0.0, nsub=1, wx=None, wy=None, events=None):
    """new (x, y, z, wx, wy, F [3, 3, n], e): the definition, vectorised over the particles.  events (a dict, optional) counts
    up (e raised), down (e lowered), held0 / held1 (substeps that ended on a plate) and lost."""
    dims = (p.nx, p.ny, p.nz)
    pnx, pny, top = float(p.nx), float(p.ny), float(p.nz - 1)
    hx, hy, hz = h / p.dx, h / p.dy, h / p.dz
    hh = (hx, hy, hz)
    aa = (0.5 * hx, 0.5 * hy, 0.5 * hz)
    x, y, z = (np.array(a, dtype=np.float64) for a in (x, y, z))
    n = x.size
    wx = np.zeros(n, np.int32) if wx is None else np.array(wx, dtype=np.int32)
    wy = np.zeros(n, np.int32) if wy is None else np.array(wy, dtype=np.int32)
    F0, e0 = identity(x, y, z)
    F = F0 if F is None else np.array(F, dtype=np.float64).reshape(3, 3, n)
    e = e0 if e is None else np.array(e, dtype=np.int32)
    ev = dict.fromkeys(("up", "down", "held0", "held1", "lost"), 0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for _ in range(nsub):
            a = np.flatnonzero(~(np.isnan(x) | np.isnan(y) | np.isnan(z)))  # the lost ones are skipped
            if a.size == 0:
                break
            xa, ya, za = x[a], y[a], z[a]
            w, G = _velocity_grad(dims, u, E, mu, xa, ya, za)
            M = [[None] * 3 for _ in range(3)]
            for s in range(3):
                for r in range(3):
                    m = aa[s] * G[s][r]
                    M[s][r] = 1.0 + m if s == r else m
            none = np.zeros(a.size, np.int32)
            x1, _, okx = T._fold(xa + aa[0] * w[0], pnx, none)
            y1, _, oky = T._fold(ya + aa[1] * w[1], pny, none)
            z1, okz = T._fold_z(za + aa[2] * w[2], top)
            ok = okx & oky & okz
            w, G = _velocity_grad(dims, u, E, mu, np.where(ok, x1, 0.0), np.where(ok, y1, 0.0), np.where(ok, z1, 0.0))
            x2, wx2, okx = T._fold(xa + hx * w[0], pnx, wx[a])
            y2, wy2, oky = T._fold(ya + hy * w[1], pny, wy[a])
            z2, okz = T._fold_z(za + hz * w[2], top)
            ok = ok & okx & oky & okz
            Fa = [[F[c, r, a] for r in range(3)] for c in range(3)]
            J = [[None] * 3 for _ in range(3)]
            for c in range(3):
                for r in range(3):
                    S = (G[c][0] * M[0][r] + G[c][1] * M[1][r]) + G[c][2] * M[2][r]
                    j = hh[c] * S
                    J[c][r] = 1.0 + j if c == r else j
            N = [[(J[c][0] * Fa[0][r] + J[c][1] * Fa[1][r]) + J[c][2] * Fa[2][r] for r in range(3)] for c in range(3)]
            N, en = _renormalise(N, e[a])
            ev["up"] += int((ok & (en > e[a])).sum())
            ev["down"] += int((ok & (en < e[a])).sum())
            ev["held0"] += int((ok & (z2 == 0.0)).sum())
            ev["held1"] += int((ok & (z2 == top)).sum())
            ev["lost"] += int((~ok).sum())
            x[a] = np.where(ok, x2, np.nan)
            y[a] = np.where(ok, y2, np.nan)
            z[a] = np.where(ok, z2, np.nan)
            wx[a] = np.where(ok, wx2, wx[a])  # a lost particle keeps its image counts ...
            wy[a] = np.where(ok, wy2, wy[a])
            e[a] = np.where(ok, en, e[a])     # ... and its e; its F is NaN
            for c in range(3):
                for r in range(3):
                    F[c, r, a] = np.where(ok, N[c][r], np.nan)
    if events is not None:
        for k, v in ev.items():
            events[k] = events.get(k, 0) + v
    return x, y, z, wx, wy, F, e


def level(F, e):
    """the level per particle by the header's rule: the sum of squares in index order, the exponent from its bit pattern"""
    F = np.asarray(F, dtype=np.float64).reshape(9, -1)
    e = np.asarray(e, dtype=np.int64).ravel()
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        trc = F[0] * F[0]
        for q in range(1, 9):
            trc = trc + F[q] * F[q]
        none = np.isnan(trc) | (trc == 0.0)
        v = np.where(none, 1.0, trc)
        sub = ((np.ascontiguousarray(v).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)) == 0
        v = np.where(sub, v * 2.0 ** 54, v)
    E = ((np.ascontiguousarray(v).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1022 - np.where(sub, 54, 0)
    return np.where(none, NO_LEVEL, 2 * e + E - 1).astype(np.int32)


def levels_hist(F, e, l_lo, nlevels):
    """(counts [nlevels + 2], none) of a record: what ekpnp_tracers_stretch_levels must give"""
    lv = level(F, e).astype(np.int64)
    has = lv != NO_LEVEL
    cell = np.clip(lv[has] - l_lo + 1, 0, nlevels + 1)
    return np.bincount(cell, minlength=nlevels + 2).astype(np.int64), int((~has).sum())


def same_record(got, want):
    """(F, e) of a stretch record: e equal, F on its bit pattern where the want is a number and NaN where it is NaN"""
    gF, ge = np.asarray(got[0]).reshape(9, -1), np.asarray(got[1])
    wF, we = np.asarray(want[0]).reshape(9, -1), np.asarray(want[1])
    if ge.dtype != np.int32 or gF.shape != wF.shape or not np.array_equal(ge, we):
        return False
    nan = np.isnan(wF)
    return bool(np.isnan(gF[nan]).all()) and T.same(gF[~nan], wF[~nan])
