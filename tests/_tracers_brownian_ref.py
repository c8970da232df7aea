"""The definition of a Brownian tracer advance (include/ekpnp.h, BROWNIAN TRACERS) transcribed into numpy, operation by operation,
on top of the transcription of the deterministic advance (tests/_tracers_ref.py), and the inputs the CPU and the GPU tests share.
Philox4x32-10 runs in uint64 arithmetic; numpy rounds every ufunc once and fuses nothing, so the transcription and
ekpnp_tracers_advance_brownian_host must agree on the float64 BIT PATTERN."""
import math

import numpy as np

import _tracers_ref as T

M32 = np.uint64(0xFFFFFFFF)
KICK_TAG = 0x80000000


def philox4x32_10(c, k0, k1):
    """c: four uint64 arrays holding 32-bit words; the ten rounds, the key bumped by the Weyl constants between them"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) for v in c)
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n1 = p1 & M32
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        n3 = p0 & M32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def kick(seed, ids, epoch):
    """r [3, n]: the draw of every id at one epoch"""
    ids = np.atleast_1d(np.asarray(ids, dtype=np.int64)).astype(np.uint64)
    e = np.uint64(int(epoch) & 0xFFFFFFFFFFFFFFFF)
    n = ids.size
    c = (ids & M32, np.full(n, e & M32), np.full(n, e >> np.uint64(32)), np.uint64(KICK_TAG) | (ids >> np.uint64(32)))
    w = philox4x32_10(c, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)
    r = []
    for a in range(3):
        v = w[a].astype(np.uint32).view(np.int32).astype(np.float64)
        s = v + 0.5
        r.append(s * 2.0 ** -31)
    return np.stack(r)


def kick_lengths(p, D, h):
    """(kx, ky, kz) in cells: t = 6 D; m = t h; q = sqrt(m) (correctly rounded); q / dx, q / dy, q / dz"""
    t = 6.0 * D
    m = t * h
    q = math.sqrt(m)
    return q / p.dx, q / p.dy, q / p.dz


def _reflect_z(z, top):
    z = np.where(z < 0.0, 0.0 - z, z)
    z = np.where(z > top, top - (z - top), z)
    return T._fold_z(z, top)


def advance(p, u, x, y, z, wx=None, wy=None, E=None, mu=0.0, D=0.0, h=0.0, nsub=1, seed=0, epoch=0, ids=None):
    """new (x, y, z, wx, wy): the definition, vectorised over the particles"""
    pnx, pny, top = float(p.nx), float(p.ny), float(p.nz - 1)
    kx, ky, kz = kick_lengths(p, D, h)
    x, y, z = (np.array(a, dtype=np.float64) for a in (x, y, z))
    n = x.size
    wx = np.zeros(n, np.int32) if wx is None else np.array(wx, dtype=np.int32)
    wy = np.zeros(n, np.int32) if wy is None else np.array(wy, dtype=np.int32)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for it in range(nsub):
            a = np.flatnonzero(~(np.isnan(x) | np.isnan(y) | np.isnan(z)))  # the lost ones are skipped
            if a.size == 0:
                break
            x1, y1, z1, wx1, wy1 = T.advance(p, u, x[a], y[a], z[a], wx[a], wy[a], E=E, mu=mu, h=h, nsub=1)   # (a)
            ok = ~np.isnan(x1)
            r = kick(seed, ids[a], epoch + it)                                                               # (b)
            t = kx * r[0]
            x2 = np.where(ok, x1 + t, 0.0)
            t = ky * r[1]
            y2 = np.where(ok, y1 + t, 0.0)
            t = kz * r[2]
            z2 = np.where(ok, z1 + t, 0.0)
            x2, wx2, okx = T._fold(x2, pnx, wx1)                                                             # (c)
            y2, wy2, oky = T._fold(y2, pny, wy1)
            z2, okz = _reflect_z(z2, top)                                                                    # (d)
            ok = ok & okx & oky & okz
            x[a] = np.where(ok, x2, np.nan)
            y[a] = np.where(ok, y2, np.nan)
            z[a] = np.where(ok, z2, np.nan)
            wx[a] = np.where(ok, wx2, wx[a])  # a lost particle keeps the image counts it had before the substep
            wy[a] = np.where(ok, wy2, wy[a])
    return x, y, z, wx, wy


# what the CPU and the GPU tests share: a diffusivity that kicks a particle by up to KICK cells per substep of T.substep(p)
KICK = 1.75
SEED = 0x9E3779B97F4A7C15


def diffusivity(p, cells=KICK):
    """D such that kx = sqrt(6 D h) / dx is about `cells` at h = T.substep(p)"""
    return (cells * p.dx) ** 2 / (6.0 * T.substep(p))


def plate_cloud(shape, n, seed):
    """T.special_cloud, and behind its special particles a few that a kick of KICK cells throws through either plate"""
    x, y, z = T.special_cloud(shape, n, seed)
    nz = shape[2]
    for k, zz in enumerate((0.0625, 0.25, nz - 1.0625, nz - 1.25, 0.0, float(nz - 1))):
        if 13 + k < n:
            z[13 + k] = zz
    return x, y, z
