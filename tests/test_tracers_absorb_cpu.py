"""CPU tests of the absorbing plates of the tracers (csrc/tracers.hip; include/ekpnp.h: ekpnp_tracers_advance_absorbing_host,
ekpnp_landings_bin): the host-only entry points, which ARE the definitions the device is held against in
tests/test_tracers_absorb_gpu.py.  No device is needed.  Every test here fails on the parent commit: the symbols do not exist there.

The advance is compared with a numpy transcription of the header's text (tests/_tracers_absorb_ref.py) on the float64 BIT PATTERN of
the five cloud arrays and of the six arrays of the landing record.  The first-passage checks have bounds that come from optional
stopping and from the sampling error of their own estimators (five standard deviations), and fixed seeds: they are deterministic."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _tracers_absorb_ref as A
import _tracers_brownian_ref as B
import _tracers_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ekpnp_tracers_advance_absorbing_host", "ekpnp_tracers_advance_absorbing", "ekpnp_landings_reset", "ekpnp_landings_get", "ekpnp_landings_bin",
         "ekpnp_landings_hist", "ekpnp_landings_map", "ekpnp_landings_save", "ekpnp_landings_load"]
N = 1000
EPOCH = 2 ** 32 - 3   # the epoch's low word wraps inside a call of seven substeps


# ---- 1. the interface ------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_mirrored(pkg):
    lib = pkg.load_library()
    for name in NAMES:
        assert name in pkg.exported_symbols()
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    assert not [n for n in pkg.exported_symbols() if n.startswith("ekpnp_group_landings") or n.startswith("ekpnp_group_tracers")]
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ekpnp.h")).read())
    for decl in ("int ekpnp_tracers_advance_absorbing(ekpnp_ctx* ctx, double mu, double D, double h, int nsub, uint64_t seed, int walls);",
                 "uint64_t seed, int64_t epoch, int walls, int64_t* land_epoch, int32_t* land_wall, double* land_x, double* land_y, int32_t* land_wx, int32_t* land_wy);",
                 "int ekpnp_landings_reset(ekpnp_ctx* ctx);",
                 "int ekpnp_landings_get(ekpnp_ctx* ctx, int64_t* epoch, int32_t* wall, double* x, double* y, int32_t* wx, int32_t* wy);",
                 "int ekpnp_landings_bin(int64_t e0, int64_t width, int nbins, int64_t epoch);",
                 "int ekpnp_landings_hist(ekpnp_ctx* ctx, int walls, int64_t e0, int64_t width, int nbins, int64_t* counts /* [nbins+2] */, int64_t* none);",
                 "int ekpnp_landings_map(ekpnp_ctx* ctx, int wall /* 1 or 2 */, int bx, int by, int64_t e_lo, int64_t e_hi, int64_t* counts /* [by][bx] */, int64_t* elsewhere);",
                 "int ekpnp_landings_save(ekpnp_ctx* ctx, const char* path);", "int ekpnp_landings_load(ekpnp_ctx* ctx, const char* path);"):
        assert decl in hdr, decl
    assert len(lib.ekpnp_tracers_advance_absorbing_host.argtypes) == 27 and len(lib.ekpnp_tracers_advance_absorbing.argtypes) == 7
    assert lib.ekpnp_tracers_advance_absorbing.argtypes[5] is C.c_uint64 and lib.ekpnp_landings_bin.argtypes[0] is C.c_int64
    for m in ("tracers_advance", "landings_get", "landings_hist", "landings_map", "landings_save", "landings_load", "landings_reset"):
        assert hasattr(pkg.Solver, m), m
    for f in ("tracers_advance_absorbing_host", "landings_bin"):
        assert callable(getattr(pkg, f)), f
    assert not [m for m in dir(pkg.Group) if "tracers" in m or "landings" in m]
    assert pkg.ABSORB_WALLS == {"bottom": 1, "top": 2, "both": 3}
    # the Brownian and the plain advance kept their signatures
    assert len(lib.ekpnp_tracers_advance_brownian_host.argtypes) == 20 and len(lib.ekpnp_tracers_advance_brownian.argtypes) == 6 and len(lib.ekpnp_tracers_advance.argtypes) == 4


# ---- 2. the advance against its transcription ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cases(pkg):
    """per lattice: the parameters, random fields with one NaN node, a cloud of N positions (some next to, on and beyond reach of the
    plates, one lost from the start, one in the NaN node's cell), a permutation of ids and a record that already holds landings; made
    once, never modified"""
    out = {}
    for k, shape in A.SHAPES.items():
        p = pkg.default_params(*shape)
        u, E = T.random_fields(shape, 171 + len(out), T.U_SCALE, T.E_SCALE)
        u[1][2, 7, 9] = np.nan                         # the particles whose stencil holds it are lost
        x, y, z = A.cloud(shape, N, 181 + len(out))
        x[40], y[40], z[40] = 8.5, 6.5, 1.5            # ... this one from the first evaluation on
        ids = np.random.default_rng(191 + len(out)).permutation(N).astype(np.int32)
        rec = A.empty_record(N)
        held = np.arange(0, N, 7)
        rec[0][held] = 2 + held % 3
        rec[1][held] = 1 + held % 2
        rec[2][held] = 1.5 + held % 5
        rec[3][held] = 2.5
        rec[4][held] = 3
        rec[5][held] = -4
        for a in (*u, *E, x, y, z, ids, *rec):
            a.setflags(write=False)
        out[k] = (p, u, E, x, y, z, ids, rec)
    return out


def _assert_same(got, want, what):
    for k, name in enumerate(("x", "y", "z")):
        assert T.same(got[k], want[k]), (what, name, np.flatnonzero(T.bits(got[k]) != T.bits(want[k]))[:5])
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]), what
    assert A.same_record(got[5:], want[5:]), (what, [np.flatnonzero(np.asarray(g) != np.asarray(w))[:5] for g, w in zip(got[5:], want[5:])])


@pytest.mark.parametrize("walls", [1, 2, 3])
@pytest.mark.parametrize("shape", ["W", "O", "R", "T"])
def test_advance_absorbing_host_equals_the_transcription_bit_for_bit(pkg, cases, shape, walls):
    p, u, E, x, y, z, ids, rec = cases[shape]
    h, D = T.substep(p), B.diffusivity(p)
    top = float(p.nz - 1)
    for mu in (0.0, T.MU):
        for nsub in (1, 7):
            kw = dict(E=E, mu=mu, D=D, h=h, nsub=nsub, seed=A.NOISE, epoch=EPOCH, ids=ids, walls=walls, record=rec)
            got = pkg.tracers_advance_absorbing_host(p, u, x, y, z, **kw)
            want = A.advance(p, u, x, y, z, **kw)
            _assert_same(got, want, (shape, walls, mu, nsub))
            # a record that already holds landings is not overwritten - and some of those particles did land again here
            held = np.arange(0, N, 7)
            for k in range(6):
                assert np.array_equal(got[5 + k][held], rec[k][held]), k
            slot_of = np.argsort(ids)
            again = held[(got[2][slot_of[held]] == 0.0) | (got[2][slot_of[held]] == top)]
            assert again.size >= 3
            # landed particles lie exactly on their plate, and every new landing has an epoch of this call
            new = np.flatnonzero((got[5] >= 0) & (rec[0] < 0))
            assert new.size >= 10 and ((got[5][new] >= EPOCH) & (got[5][new] <= EPOCH + nsub)).all()
            zl = got[2][slot_of[new]]
            assert np.array_equal(zl, np.where(got[6][new] == 1, 0.0, top)) and ((got[6][new] & walls) != 0).all()
            assert T.same(got[7][new], got[0][slot_of[new]]) and T.same(got[8][new], got[1][slot_of[new]])
            assert np.array_equal(got[9][new], got[3][slot_of[new]]) and np.array_equal(got[10][new], got[4][slot_of[new]])
    # the defaults of the wrapper: ids 0 .. n-1, an empty record, both plates
    got = pkg.tracers_advance_absorbing_host(p, u, x, y, z, D=D, h=h, nsub=3, seed=5)
    _assert_same(got, A.advance(p, u, x, y, z, D=D, h=h, nsub=3, seed=5), (shape, "defaults"))


def test_every_case_of_the_definition_did_happen(pkg, cases):
    p, u, E, x, y, z, ids, _ = cases["W"]
    h, D = T.substep(p), B.diffusivity(p)
    top = float(p.nz - 1)
    for walls in (1, 2, 3):
        ev = {}
        kw = dict(E=E, mu=T.MU, D=D, h=h, nsub=7, seed=A.NOISE, epoch=11, ids=ids, walls=walls)
        want = A.advance(p, u, x, y, z, events=ev, **kw)
        got = pkg.tracers_advance_absorbing_host(p, u, x, y, z, **kw)
        _assert_same(got, want, walls)
        if walls & 1:
            assert ev["kick1"] >= 10 and ev["reflect1"] == 0          # a landing on the bottom plate by a kick
        else:
            assert ev["kick1"] == 0 and ev["reflect1"] >= 10          # a reflection at the plate that does not absorb
        if walls & 2:
            assert ev["kick2"] >= 10 and ev["reflect2"] == 0
        else:
            assert ev["kick2"] == 0 and ev["reflect2"] >= 10
        # a particle on the plate at entry is recorded with the call's epoch, where it stands, and is not moved
        on = np.flatnonzero(((z <= 0.0) & bool(walls & 1)) | ((z >= top) & bool(walls & 2)))
        assert on.size >= 2 and ev["stuck"] == on.size
        assert (got[5][ids[on]] == 11).all() and T.same(got[7][ids[on]], x[on]) and T.same(got[8][ids[on]], y[on])
        for k, a in enumerate((x, y, z)):
            assert T.same(got[k][on], a[on])
        # lost particles: the one lost from the start, the ones the NaN node took; none of them has a landing
        lost = np.flatnonzero(np.isnan(got[0]))
        assert np.isnan(x[12]) and 12 in lost and 40 in lost and ev["lost"] >= 1 and (got[5][ids[lost]] == -1).all() and (got[6][ids[lost]] == 0).all()
        # a wrap in x and one in y before a landing
        assert (got[9] != 0).any() and (got[10] != 0).any()
        assert ((got[5] >= 0) == (got[6] != 0)).all() and (np.isnan(got[7]) == (got[5] < 0)).all()


def test_drift_alone_deposits(pkg):
    """D == 0: a field that pushes into a plate lands the particles there, by the hold of the midpoint substep; nothing is drawn"""
    shape = (12, 10, 9)
    p = pkg.default_params(*shape)
    n = 200
    rng = np.random.default_rng(5)
    x, y, z = rng.uniform(0, 12, n), rng.uniform(0, 10, n), rng.uniform(0.5, 7.5, n)
    zero = np.zeros((9, 10, 12))
    h = p.dz / 1e-3   # a cell per substep
    for sign, wall in ((-1.0, 1), (1.0, 2)):
        for mu, u, E in ((0.0, [zero, zero, zero + sign * 1e-3], None), (1e-8, [zero, zero, zero], [zero, zero, zero + sign * 1e5])):
            ev = {}
            kw = dict(E=E, mu=mu, D=0.0, h=h, nsub=5, seed=3, epoch=100, walls=3)
            got = pkg.tracers_advance_absorbing_host(p, u, x, y, z, **kw)
            _assert_same(got, A.advance(p, u, x, y, z, events=ev, **kw), (sign, mu))
            key = "drift%d" % wall
            assert ev[key] == (got[6] == wall).sum() > 50 and sum(v for k, v in ev.items() if k != key) == 0
            assert (got[6][got[5] >= 0] == wall).all() and (got[5] < 0).sum() > 10   # five cells: the far ones are still under way
            d = np.where(got[5] >= 0)[0]
            dist = z[d] if wall == 1 else 8.0 - z[d]
            assert np.array_equal(got[5][d], 100 + np.ceil(dist).astype(np.int64))   # one cell per substep
            assert T.same(got[7][d], x[d]) and T.same(got[8][d], y[d])
    # with walls that do not hold the plate it drifts to, it is held there as by a plain advance, and nothing lands
    got = pkg.tracers_advance_absorbing_host(p, [zero, zero, zero - 1e-3], x, y, z, D=0.0, h=h, nsub=9, walls=2)
    assert (got[2] == 0.0).all() and (got[5] == -1).all()


# ---- 3. invariants -----------------------------------------------------------------------------------------------------

def _inside(x, y, z, top):
    """the shared cloud with everybody strictly between the plates"""
    z = np.array(z)
    z[z <= 0.0] = 0.5
    z[z >= top] = top - 0.5
    return x, y, z


@pytest.mark.parametrize("walls", [1, 2, 3])
def test_until_it_lands_a_particle_has_the_bits_of_the_brownian_advance(pkg, cases, walls):
    p, u, E, x, y, z, ids, _ = cases["T"]
    top = float(p.nz - 1)
    x, y, z = _inside(x, y, z, top)
    kw = dict(E=E, mu=T.MU, D=B.diffusivity(p), h=T.substep(p), nsub=7, seed=A.NOISE, epoch=5, ids=ids)
    got = pkg.tracers_advance_absorbing_host(p, u, x, y, z, walls=walls, **kw)
    brown = pkg.tracers_advance_brownian_host(p, u, x, y, z, **kw)
    free = got[5][ids] < 0
    assert 100 < free.sum() < N - 100
    for k in range(3):
        assert T.same(got[k][free], brown[k][free]), k
    assert np.array_equal(got[3][free], brown[3][free]) and np.array_equal(got[4][free], brown[4][free])
    landed = ~free
    assert np.array_equal(got[2][landed], np.where(got[6][ids][landed] == 1, 0.0, top))   # exactly 0.0 or top
    assert not T.same(got[0][landed], brown[0][landed])                                   # their remaining substeps were not taken


def test_two_calls_equal_one_and_a_stuck_particle_is_left_alone(pkg, cases):
    p, u, E, x, y, z, ids, rec = cases["W"]
    top = float(p.nz - 1)
    kw = dict(E=E, mu=T.MU, D=B.diffusivity(p), h=T.substep(p), seed=A.NOISE, ids=ids, walls=3)
    whole = pkg.tracers_advance_absorbing_host(p, u, x, y, z, nsub=7, epoch=9, record=rec, **kw)
    first = pkg.tracers_advance_absorbing_host(p, u, x, y, z, nsub=3, epoch=9, record=rec, **kw)
    second = pkg.tracers_advance_absorbing_host(p, u, *first[:5], nsub=4, epoch=12, record=first[5:], **kw)
    _assert_same(second, whole, "3 + 4")
    assert not A.same_record(first[5:], whole[5:])   # the second call did record landings
    # a stuck particle's entries are untouched by the next absorbing call, whatever its seed
    stuck = (whole[2] == 0.0) | (whole[2] == top)
    assert stuck.sum() > 100
    third = pkg.tracers_advance_absorbing_host(p, u, *whole[:5], nsub=5, epoch=16, record=whole[5:], **dict(kw, seed=77))
    for k in range(3):
        assert T.same(third[k][stuck], whole[k][stuck]), k
    assert np.array_equal(third[3][stuck], whole[3][stuck]) and np.array_equal(third[4][stuck], whole[4][stuck])
    had = whole[5] >= 0
    for k in range(6):
        assert np.array_equal(third[5 + k][had], whole[5 + k][had], equal_nan=True), k


def test_a_brownian_advance_moves_a_stuck_particle_and_the_record_stays(pkg, cases):
    p, u, E, x, y, z, ids, _ = cases["W"]
    top = float(p.nz - 1)
    kw = dict(E=E, mu=T.MU, D=B.diffusivity(p), h=T.substep(p), seed=A.NOISE, ids=ids)
    a = pkg.tracers_advance_absorbing_host(p, u, x, y, z, nsub=7, epoch=0, walls=3, **kw)
    stuck = (a[2] == 0.0) | (a[2] == top)
    b = pkg.tracers_advance_brownian_host(p, u, *a[:5], nsub=2, epoch=7, **kw)
    moved = stuck & ~np.isnan(b[2])
    assert moved.sum() > 100 and (b[2][moved] > 0.0).all() and (b[2][moved] < top).all()
    c = pkg.tracers_advance_absorbing_host(p, u, *b, nsub=7, epoch=9, walls=3, record=a[5:], **kw)
    had = a[5] >= 0
    back = had[ids] & ((c[2] == 0.0) | (c[2] == top))
    assert back.sum() > 20                                # they landed a second time ...
    for k in range(6):
        assert np.array_equal(c[5 + k][had], a[5 + k][had]), k   # ... and the record keeps the first landing
    assert (c[5][~had] >= 9).sum() > 0
    plain = pkg.tracers_advance_host(p, u, *a[:5], E=E, mu=T.MU, h=T.substep(p), nsub=1)   # a plain advance moves them too
    assert not T.same(plain[0][stuck], a[0][stuck])


# ---- 4. the bin rule and the refusals ----------------------------------------------------------------------------------

def _bin(e0, width, nbins, e):
    return 0 if e < e0 else min(1 + (e - e0) // width, nbins + 1)


def test_landings_bin_is_integer_arithmetic_at_every_edge(pkg):
    big = 2 ** 62
    for e0, width, nbins in ((0, 1, 1), (5, 1, 4), (5, 3, 4), (0, 7, 4096), (17, 1000, 64), (big - 50, 9, 11), (3, big // 2, 2), (big, 1, 4096), (0, 2 ** 63 - 1, 1)):
        edges = {e0 - 1, e0, e0 + 1, e0 + width - 1, e0 + width, e0 + nbins * width - 1, e0 + nbins * width, e0 + nbins * width + 1, e0 + 2 * width - 1, e0 + 2 * width,
                 -1, 0, 1, big - 1, big, big + 1, 2 ** 63 - 1}
        for e in sorted(v for v in edges if -1 <= v < 2 ** 63):
            assert pkg.landings_bin(e0, width, nbins, e) == _bin(e0, width, nbins, e), (e0, width, nbins, e)
    assert pkg.landings_bin(5, 3, 4, 4) == 0 and pkg.landings_bin(5, 3, 4, 5) == 1 and pkg.landings_bin(5, 3, 4, 7) == 1 and pkg.landings_bin(5, 3, 4, 8) == 2
    assert pkg.landings_bin(5, 3, 4, 16) == 4 and pkg.landings_bin(5, 3, 4, 17) == 5 and pkg.landings_bin(5, 3, 4, 2 ** 62) == 5
    e = np.arange(-1, 40)
    assert np.array_equal(pkg.landings_bin(5, 3, 4, e), [_bin(5, 3, 4, int(v)) for v in e])
    assert np.array_equal(A.hist([e, np.where(e >= 0, 1, 0)], 1, 5, 3, 4)[0], np.bincount(pkg.landings_bin(5, 3, 4, e[1:]), minlength=6))
    L = pkg.load_library()
    for args, msg in (((-1, 1, 1, 0), b"e0 = -1"), ((0, 0, 1, 0), b"width = 0"), ((0, -3, 1, 0), b"width = -3"), ((0, 1, 0, 0), b"nbins = 0"), ((0, 1, 4097, 0), b"nbins = 4097")):
        assert L.ekpnp_landings_bin(*args) == -1 and msg in L.ekpnp_last_error(None), args
    with pytest.raises(pkg.EkpnpError) as err:
        pkg.landings_bin(0, 1, 5000, 3)
    assert "nbins = 5000" in str(err.value)


def test_refusals_give_the_offending_number(pkg):
    L = pkg.load_library()
    W = A.SHAPES["W"]
    p = pkg.default_params(*W)
    a = np.full(10, 2.5)
    w = np.zeros(10, dtype=np.int32)
    ids = np.arange(10, dtype=np.int32)
    u = np.zeros((W[2], W[1], W[0]))
    rec = A.empty_record(10)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    #        0           1       2       3       4     5     6     7   8         9       10      11      12      13      14   15    16     17 18 19 20 21 ..
    args = [C.byref(p), ptr(u), ptr(u), ptr(u), None, None, None, 10, ptr(ids), ptr(a), ptr(a), ptr(a), ptr(w), ptr(w), 0.0, 0.5, 0.25, 1, 7, 0, 3, *[ptr(r) for r in rec]]
    assert L.ekpnp_tracers_advance_absorbing_host(*args) == 0   # mu == 0: the E arrays are not needed
    cases = [(15, -1.5, b"D = -1.5"), (15, math.nan, b"D = nan"), (15, math.inf, b"D = inf"), (16, -0.25, b"D*h = -0.125"),
             (17, 0, b"nsub = 0"), (17, -2, b"nsub = -2"), (17, 4097, b"nsub = 4097"), (14, math.inf, b"mu = inf"), (16, math.nan, b"h = nan"),
             (16, math.inf, b"h = inf"), (19, -3, b"epoch = -3"), (7, -1, b"n = -1"), (7, (1 << 28) + 1, b"n = 268435457"), (14, 1e-8, b"NULL"),
             (20, 0, b"walls = 0"), (20, 4, b"walls = 4"), (20, -1, b"walls = -1")]
    for k, v, msg in cases:
        bad = list(args)
        bad[k] = v
        assert L.ekpnp_tracers_advance_absorbing_host(*bad) == 1 and msg in L.ekpnp_last_error(None), (k, v, L.ekpnp_last_error(None))
    for k in (0, 1, 9, 13, 21, 22, 23, 24, 25, 26):
        bad = list(args)
        bad[k] = None
        assert L.ekpnp_tracers_advance_absorbing_host(*bad) == 1 and b"NULL" in L.ekpnp_last_error(None), k
    # the record: a wall outside 0 .. 2; an epoch < 0 with a wall; the ids: outside 0 .. n-1 - each with the first offending entry
    for k, field, v, msg in ((1, 4, 3, b"id 4: wall = 3"), (1, 6, -1, b"id 6: wall = -1"), (1, 2, 2, b"id 2: epoch = -1 with wall = 2")):
        r = A.empty_record(10)
        r[k][field] = v
        bad = args[:21] + [ptr(q) for q in r]
        assert L.ekpnp_tracers_advance_absorbing_host(*bad) == 1 and msg in L.ekpnp_last_error(None), L.ekpnp_last_error(None)
    r = A.empty_record(10)
    r[0][3] = -7
    r[1][3] = 1
    assert L.ekpnp_tracers_advance_absorbing_host(*(args[:21] + [ptr(q) for q in r])) == 1 and b"id 3: epoch = -7 with wall = 1" in L.ekpnp_last_error(None)
    for v in (10, -1):
        wrong = ids.copy()
        wrong[5] = v
        bad = list(args)
        bad[8] = ptr(wrong)
        assert L.ekpnp_tracers_advance_absorbing_host(*bad) == 1 and b"slot 5 holds id %d" % v in L.ekpnp_last_error(None)
    thin = pkg.default_params(8, 8, 8)
    thin.nz = 2
    bad = list(args)
    bad[0] = C.byref(thin)
    assert L.ekpnp_tracers_advance_absorbing_host(*bad) == 1 and b"nz = 2" in L.ekpnp_last_error(None)
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.tracers_advance_absorbing_host(p, [u, u, u], a, a, a, D=1e-9, h=1e-3, walls=4)
    assert "walls = 4" in str(e.value) and "status 1" in str(e.value)
    with pytest.raises(ValueError):
        pkg.tracers_advance_absorbing_host(p, [u, u, u], a, a, a, D=1e-9, h=1e-3, walls="sides")
    # the context calls refuse a NULL context
    assert L.ekpnp_tracers_advance_absorbing(None, 0.0, 0.0, 0.0, 1, 0, 3) == 1 and L.ekpnp_landings_reset(None) == 1
    assert L.ekpnp_landings_get(None, *[None] * 6) == 1 and L.ekpnp_landings_save(None, b"x") == 1 and L.ekpnp_landings_load(None, b"x") == 1
    one = C.c_int64()
    assert L.ekpnp_landings_hist(None, 3, 0, 1, 1, ptr(np.zeros(3, np.int64)), C.byref(one)) == 1
    assert L.ekpnp_landings_map(None, 1, 1, 1, 0, 1, ptr(np.zeros(1, np.int64)), C.byref(one)) == 1


# ---- 5. first passage against theory -----------------------------------------------------------------------------------

def test_first_passage_obeys_optional_stopping(pkg):
    """Zero fields, both plates absorbing, every particle started at one height z0 strictly inside, a kick length of kz = 0.5 cells
    in a channel of 8.  Until the exit z is a martingale whose increments lie in (-kz, kz) with variance kz^2/3 (the kick is
    kz * r with r uniform in (-1, 1)), and the exit height z_tau - before the plate keeps it - lies within kz beyond a plate.
    Optional stopping of z:  z0 = E z_tau  gives  (z0 - kz)/top <= P(top) <= (z0 + kz)/top.
    Optional stopping of z^2 - t kz^2/3:  E[tau] kz^2/3 = E[(z_tau - z0)^2], and from mid-channel a <= |z_tau - z0| < a + kz with
    a = top/2:  3 a^2/kz^2 <= E[tau] <= 3 (a + kz)^2/kz^2.
    Sampling: P within 5 sqrt(p (1-p)/n) at p = z0/top; the mean epoch within 5 sigma_tau/sqrt(n), sigma_tau from the continuous
    exit time of a Brownian motion of variance rate s^2 = kz^2/3 from the middle of (-a, a): E tau = a^2/s^2, E tau^2 = 5 a^4/(3 s^4)
    (the even solution of s^2 v''/2 = -2 (a^2 - x^2)/s^2 with v(+-a) = 0 at x = 0), so Var tau = 2 a^4/(3 s^4) - which is
    L^4/(96 D^2) for a gap L = 2 a and s^2 = 2 D.
    The slowest mode of the survival decays by exp(-pi^2 s^2/(8 a^2)) = exp(-0.0064) per substep: after 4096 substeps 4e-12 of a
    cloud is left, so that the definition itself leaves no survivor among 4096 particles; none == 0 is a CONDITION of the test."""
    shape = (8, 8, 9)
    p = pkg.default_params(*shape)
    top, kz, n = 8.0, 0.5, 4096
    h = 1.0
    D = (kz * p.dz) ** 2 / (6.0 * h)
    assert abs(B.kick_lengths(p, D, h)[2] - kz) < 1e-12
    zero = np.zeros((9, 8, 8))
    rng = np.random.default_rng(11)
    x, y = rng.uniform(0, 8, n), rng.uniform(0, 8, n)
    for z0 in (4.0, 2.0):
        got = pkg.tracers_advance_absorbing_host(p, [zero, zero, zero], x, y, np.full(n, z0), D=D, h=h, nsub=4096, seed=2024, walls=3)
        counts, none = A.hist(got[5:], 3, 0, 1, 4096)
        assert none == 0 and counts.sum() == n and counts[0] == 0    # the condition: everybody has landed
        share = (got[6] == 2).mean()
        q = z0 / top
        slack = 5.0 * math.sqrt(q * (1.0 - q) / n)
        print("z0", z0, "share on top", share, "bounds", (z0 - kz) / top - slack, (z0 + kz) / top + slack)
        assert (z0 - kz) / top - slack <= share <= (z0 + kz) / top + slack
        if z0 == 4.0:
            a, s2 = top / 2.0, kz * kz / 3.0
            sigma = math.sqrt(2.0 * a ** 4 / (3.0 * s2 * s2))
            mean = got[5].mean()
            slack = 5.0 * sigma / math.sqrt(n)
            print("mean epoch", mean, "bounds", a * a / s2 - slack, (a + kz) ** 2 / s2 + slack)
            assert a * a / s2 - slack <= mean <= (a + kz) ** 2 / s2 + slack
            assert (got[5] >= 8).all()   # nobody crosses four cells in fewer than eight kicks of half a cell
