"""The definition of an absorbing tracer advance (include/ekpnp.h, ABSORBING PLATES) transcribed into numpy, operation by operation,
on top of the transcriptions of the deterministic advance (tests/_tracers_ref.py: the midpoint substep, the folds) and of the
Brownian one (tests/_tracers_brownian_ref.py: the draw, the kick lengths), and the inputs the CPU and the GPU tests share.  numpy
rounds every ufunc once and fuses nothing, so the transcription and ekpnp_tracers_advance_absorbing_host must agree on the float64
BIT PATTERN of the cloud and of the landing record."""
import numpy as np

import _tracers_brownian_ref as B
import _tracers_ref as T

RECORD = ("land_epoch", "land_wall", "land_x", "land_y", "land_wx", "land_wy")
RECORD_TYPES = (np.int64, np.int32, np.float64, np.float64, np.int32, np.int32)


def empty_record(n):
    """nobody has landed: epoch -1, wall 0, x and y NaN, image counts 0"""
    return [np.full(n, -1, np.int64), np.zeros(n, np.int32), np.full(n, np.nan), np.full(n, np.nan), np.zeros(n, np.int32), np.zeros(n, np.int32)]


def on_plate(walls, z, top):
    """1: on the absorbing bottom plate, else 2: on the absorbing top plate, else 0"""
    bottom = bool(walls & 1) & (z <= 0.0)
    upper = bool(walls & 2) & (z >= top)
    return np.where(bottom, 1, np.where(upper, 2, 0)).astype(np.int32)


def _absorb_z(z, top, walls):
    """(d): lost if not finite; through an absorbing plate: the plate; through the other: reflected; then the hold of step 6"""
    ok = np.isfinite(z)
    below, above = z < 0.0, z > top
    z = np.where(below, 0.0 if walls & 1 else 0.0 - z, z)
    above = z > top
    z = np.where(above, top if walls & 2 else top - (z - top), z)
    z, _ = T._fold_z(z, top)
    return z, ok, below, above


def _land(rec, ids, who, epoch, wall, x, y, wx, wy):
    """a FIRST-passage record: entries that hold a landing are left alone"""
    new = who[rec[0][ids[who]] < 0]
    k = ids[new]
    rec[0][k] = epoch
    rec[1][k] = wall[new]
    rec[2][k] = x[new]
    rec[3][k] = y[new]
    rec[4][k] = wx[new]
    rec[5][k] = wy[new]


def advance(p, u, x, y, z, wx=None, wy=None, E=None, mu=0.0, D=0.0, h=0.0, nsub=1, seed=0, epoch=0, ids=None, walls=3, record=None, events=None):
    """new (x, y, z, wx, wy, land_epoch, land_wall, land_x, land_y, land_wx, land_wy): the definition, vectorised over the
    particles.  events (a dict, optional) counts what happened: stuck, drift1, drift2, kick1, kick2 (landings by cause and wall),
    reflect1, reflect2 (reflections at a plate that does not absorb) and lost."""
    pnx, pny, top = float(p.nx), float(p.ny), float(p.nz - 1)
    kx, ky, kz = B.kick_lengths(p, D, h)
    x, y, z = (np.array(a, dtype=np.float64) for a in (x, y, z))
    n = x.size
    wx = np.zeros(n, np.int32) if wx is None else np.array(wx, dtype=np.int32)
    wy = np.zeros(n, np.int32) if wy is None else np.array(wy, dtype=np.int32)
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    rec = empty_record(n) if record is None else [np.array(a, dtype=t) for a, t in zip(record, RECORD_TYPES)]
    ev = dict.fromkeys(("stuck", "drift1", "drift2", "kick1", "kick2", "reflect1", "reflect2", "lost"), 0)
    with np.errstate(invalid="ignore", over="ignore"):
        alive = ~(np.isnan(x) | np.isnan(y) | np.isnan(z))
        stuck = alive & (on_plate(walls, z, top) != 0)
        who = np.flatnonzero(stuck)                      # no substep, no draw, the cloud is not written: the call's epoch
        ev["stuck"] += int((rec[0][ids[who]] < 0).sum())
        _land(rec, ids, who, epoch, on_plate(walls, z, top), x, y, wx, wy)
        moving = alive & ~stuck
        for it in range(nsub):
            a = np.flatnonzero(moving)
            if a.size == 0:
                break
            x1, y1, z1, wx1, wy1 = T.advance(p, u, x[a], y[a], z[a], wx[a], wy[a], E=E, mu=mu, h=h, nsub=1)     # (a)
            ok = ~np.isnan(x1)
            wall_a = np.where(ok, on_plate(walls, np.where(ok, z1, 1.0), top), 0)   # drift into the wall: no kick follows
            r = B.kick(seed, ids[a], epoch + it)                                                               # (b)
            t = kx * r[0]
            x2 = np.where(ok, x1 + t, 0.0)
            t = ky * r[1]
            y2 = np.where(ok, y1 + t, 0.0)
            t = kz * r[2]
            z2 = np.where(ok, z1 + t, 0.0)
            x2, wx2, okx = T._fold(x2, pnx, wx1)                                                             # (c)
            y2, wy2, oky = T._fold(y2, pny, wy1)
            z2, okz, below, above = _absorb_z(z2, top, walls)                                                # (d)
            ok2 = ok & okx & oky & okz
            wall_d = np.where(ok2, on_plate(walls, z2, top), 0)
            drift = wall_a != 0
            kept = ok & (drift | ok2)
            xn = np.where(drift, x1, x2)
            yn = np.where(drift, y1, y2)
            zn = np.where(drift, z1, z2)
            wxn = np.where(drift, wx1, wx2)
            wyn = np.where(drift, wy1, wy2)
            wall = np.where(drift, wall_a, wall_d).astype(np.int32)
            x[a] = np.where(kept, xn, np.nan)
            y[a] = np.where(kept, yn, np.nan)
            z[a] = np.where(kept, zn, np.nan)
            wx[a] = np.where(kept, wxn, wx[a])           # a lost particle keeps the image counts it had before the substep
            wy[a] = np.where(kept, wyn, wy[a])
            landed = kept & (wall != 0)
            full_wall = np.zeros(n, np.int32)
            full_wall[a] = wall
            _land(rec, ids, a[landed], epoch + it + 1, full_wall, x, y, wx, wy)
            moving[a[landed | ~kept]] = False
            kicked = ok & ~drift & ok2
            ev["lost"] += int((~kept).sum())
            ev["drift1"] += int((drift & (wall_a == 1)).sum())
            ev["drift2"] += int((drift & (wall_a == 2)).sum())
            ev["kick1"] += int((kicked & (wall_d == 1)).sum())
            ev["kick2"] += int((kicked & (wall_d == 2)).sum())
            if not walls & 1:
                ev["reflect1"] += int((kicked & below).sum())
            if not walls & 2:
                ev["reflect2"] += int((kicked & above).sum())
    if events is not None:
        for k, v in ev.items():
            events[k] = events.get(k, 0) + v
    return (x, y, z, wx, wy, *rec)


def same_record(got, want):
    """the six arrays of a landing record: the integers equal, x and y on their bit pattern where a landing is held and NaN elsewhere
    (the device clears with all bits set, numpy's NaN has other bits)"""
    ge, gw, gx, gy, gwx, gwy = got
    we, ww, wx_, wy_, wwx, wwy = want
    if not (ge.dtype == np.int64 and gw.dtype == np.int32 and gwx.dtype == np.int32 and gwy.dtype == np.int32):
        return False
    if not (np.array_equal(ge, we) and np.array_equal(gw, ww) and np.array_equal(gwx, wwx) and np.array_equal(gwy, wwy)):
        return False
    held = np.asarray(we) >= 0
    return (T.same(np.asarray(gx)[held], np.asarray(wx_)[held]) and T.same(np.asarray(gy)[held], np.asarray(wy_)[held])
            and bool(np.isnan(np.asarray(gx)[~held]).all()) and bool(np.isnan(np.asarray(gy)[~held]).all()))


def hist(record, walls, e0, width, nbins):
    """(counts [nbins + 2], none) of a record by integer arithmetic: what ekpnp_landings_hist must give"""
    e, w = np.asarray(record[0], dtype=np.int64), np.asarray(record[1])
    counted = (w != 0) & ((walls >> np.maximum(w - 1, 0)) & 1).astype(bool)
    ep = e[counted]
    cell = np.where(ep < e0, 0, np.minimum(1 + (ep - e0) // width, nbins + 1))
    return np.bincount(cell, minlength=nbins + 2).astype(np.int64), int(e.size - counted.sum())


def deposit(dims, record, wall, bx, by, e_lo, e_hi):
    """(counts [by, bx], elsewhere) of a record by ekpnp_tracers_cell's rule: what ekpnp_landings_map must give"""
    e, w = np.asarray(record[0], dtype=np.int64), np.asarray(record[1])
    counted = (w == wall) & (e >= e_lo) & (e <= e_hi)
    cell = T.cell(dims, (bx, by, 1), np.asarray(record[2])[counted], np.asarray(record[3])[counted], np.zeros(int(counted.sum())))
    return np.bincount(cell, minlength=bx * by).astype(np.int64).reshape(by, bx), int(e.size - counted.sum())


# what the CPU and the GPU tests share
SHAPES = {"W": (70, 66, 13), "O": (35, 33, 5), "R": (40, 12, 17), "T": (70, 66, 17)}
NOISE = 0xABCDE0123456789


def cloud(shape, n, seed):
    """B.plate_cloud (particles at 0.0625 and 0.25 from either plate, on both plates, lost from the start), and behind them a few
    that sit next to a plate AND next to a periodic edge, so that a landing follows a wrap in x or in y"""
    x, y, z = B.plate_cloud(shape, n, seed)
    nx, ny, nz = shape
    corner = [(0.0625, 3.5, 0.125), (nx - 0.0625, 4.5, nz - 1.125), (5.5, 0.0625, 0.125), (6.5, ny - 0.0625, nz - 1.125),
              (0.03125, 0.03125, 0.0625), (nx - 0.03125, ny - 0.03125, nz - 1.0625)]
    for k, (a, b, c) in enumerate(corner):
        if 19 + k < n:
            x[19 + k], y[19 + k], z[19 + k] = a, b, c
    return x, y, z
