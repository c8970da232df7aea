"""GPU tests of the x-y power spectra per z plane (csrc/spectrum.hip; include/ekpnp.h: ekpnp_spectrum_plane, ekpnp_spectrum,
ekpnp_spectrum_* and the ekpnp_group_* spellings; `ekpnp_main --spectrum-every N`).

The powers P = w |F|^2 are held against a DFT in numpy.longdouble (cos / sin matrices with the phase reduced in integers) with
the bound |P - P_exact| <= 4 u, u = log2(nx ny) 2**-53 nx ny sum v^2: the first-order error of an FFT's coefficient times 2|F|;
numpy.fft.rfft2 in float64 stays within 0.2 u of that reference on these shapes, and the library measured 0.15 u on an MI355X
(Parseval: 0.25 u; the test prints both figures).  Shells are held against math.fsum of the library's own plane binned with the
library's own table, with the first-order bound of any order of additions; peaks, the bits across buffer modes, decompositions and
batch slots, and the ring against a twin's synchronous values are held exactly."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
R = (40, 12, 17)
W = (70, 66, 13)   # factors 2.5.7 and 2.3.11, Lx != Ly, slabs of 3
V = (128, 36, 9)   # rows of a multiple of 64, slabs of 4 + 5
CASES = {"W": (W, 3, (2, 3)), "V": (V, 2, (2,))}
OFFSET_PLANE = 5   # uz on this plane: a mean 5000 times its fluctuation


def _params(pkg, shape, in_place=0):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    p.in_place = in_place
    return p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _random_fields(pkg, shape_zyx, seed):
    rng = np.random.default_rng(seed)
    scale = {"rho": 1000.0, "c": 30.0, "cn": 30.0, "phi": 5e-3, "T": 1.0, "Ex": 1e5, "Ey": 1e5, "Ez": 1e5}
    f = {n: scale.get(n, 1e-3) * rng.uniform(-1.0, 1.0, size=shape_zyx) for n in pkg.FIELDS}
    f["uz"][OFFSET_PLANE] += 5000.0 * 1e-3
    return f


def _exact_power(v):
    """P of rfft2's layout from a DFT in numpy.longdouble, the phases reduced in integers"""
    ny, nx = v.shape
    nxh = nx // 2 + 1
    ld = np.longdouble
    twopi = ld(8) * np.arctan(ld(1))
    kx = (np.arange(nxh)[:, None] * np.arange(nx)[None, :]) % nx
    ky = (np.arange(ny)[:, None] * np.arange(ny)[None, :]) % ny
    thx, thy = twopi * kx.astype(ld) / ld(nx), twopi * ky.astype(ld) / ld(ny)
    cx, sx, cy, sy = np.cos(thx), np.sin(thx), np.cos(thy), np.sin(thy)
    vl = v.astype(ld)
    ar, ai = vl @ cx.T, -(vl @ sx.T)                    # [ny][nxh]: the x transform
    fr, fi = cy @ ar + sy @ ai, cy @ ai - sy @ ar       # (cy - i sy) (ar + i ai)
    w = np.full(nxh, 2.0, dtype=ld)
    w[0] = 1.0
    if nx % 2 == 0:
        w[nx // 2] = 1.0
    return w[None, :] * (fr * fr + fi * fi)


def _sum_squares(v):
    """sum v^2, exact, then rounded once"""
    return float(sum(Fraction(float(x)) ** 2 for x in v.ravel()))


def _u(v):
    ny, nx = v.shape
    return math.log2(nx * ny) * 2.0 ** -53 * nx * ny * _sum_squares(v)


@pytest.fixture(scope="module", params=list(CASES))
def random_case(pkg, request):
    """random fields of W or V and, on a two-buffer context, P of every plane and shells and peaks of all planes of uz and phi
    (computed once, never modified)"""
    shape, nranks, groups = CASES[request.param]
    nz = shape[2]
    f = _random_fields(pkg, (shape[2], shape[1], shape[0]), 31)
    with pkg.Solver(_params(pkg, shape)) as s:
        s.set_fields(f)
        table = s.spectrum_shells()
        planes = {name: np.array([s.spectrum_plane(name, z) for z in range(nz)]) for name in ("uz", "phi")}
        full = {name: s.spectrum(name) for name in ("uz", "phi")}
    return shape, nranks, groups, f, table, planes, full


# ---- 1. against the exact transform ------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uz", "phi"])
def test_powers_against_the_exact_transform_and_parseval(pkg, random_case, name):
    shape, _, _, f, _, planes, _ = random_case
    nx, ny, nz = shape
    worst = worst_parseval = 0.0
    for z in range(nz):
        v = f[name][z]
        if name == "uz" and z == OFFSET_PLANE:
            assert abs(v.mean()) > 4000.0 * np.abs(v - v.mean()).max()
        got = planes[name][z]
        assert got.shape == (ny, nx // 2 + 1)
        u = _u(v)
        err = np.abs(got.astype(np.longdouble) - _exact_power(v))
        worst = max(worst, float(err.max()) / u)
        assert (err <= 4.0 * u).all(), (name, z, float(err.max()) / u)
        perr = abs(math.fsum(got.ravel().tolist()) - nx * ny * _sum_squares(v))
        worst_parseval = max(worst_parseval, perr / u)
        assert perr <= 4.0 * u, (name, z, perr / u)
    print(f"{shape} {name}: largest |P - P_exact| / u = {worst:.3e}, largest Parseval error / u = {worst_parseval:.3e}")


# ---- 2. shells and peaks against the library's own plane ---------------------------------------------------

def _numpy_peak(P):
    ny, nxh = P.shape
    flat = np.where(P.ravel() > 0.0, P.ravel(), -np.inf)  # a NaN or a zero is no candidate ...
    flat[0] = -np.inf                                  # ... nor is (0, 0)
    if flat.max() == -np.inf:
        return (0.0, 0.0, 0.0)
    i = int(np.argmax(flat))                           # the first of equals: the smallest linear index
    m, n = i % nxh, i // nxh
    return (float(m), float(n - ny if n > ny // 2 else n), float(P.ravel()[i]))


@pytest.mark.parametrize("name", ["uz", "phi"])
def test_shells_and_peak_of_a_chosen_plane_against_its_own_powers(pkg, random_case, name):
    shape, _, _, f, (shell_of, count), planes, full = random_case
    nz = shape[2]
    nshell = len(count)
    worst = 0.0
    with pkg.Solver(_params(pkg, shape)) as s:
        s.set_fields(f)
        for z in (0, 1, OFFSET_PLANE, nz - 1):
            shells, peaks = s.spectrum(name, [z])
            assert shells.shape == (1, nshell) and peaks.shape == (1, 3)
            P = planes[name][z]
            for k in range(nshell):
                terms = P[shell_of == k].tolist()
                assert len(terms) == count[k]
                bound = (count[k] + 8) * 2.0 ** -53 * math.fsum(abs(t) for t in terms)
                err = abs(shells[0, k] - math.fsum(terms))
                assert err <= bound, (name, z, k, shells[0, k], err, bound)
                if bound > 0.0:
                    worst = max(worst, err / bound)
            assert tuple(peaks[0]) == _numpy_peak(P), (name, z)
            assert _same(shells[0], full[name][0][z]) and _same(peaks[0], full[name][1][z])
    print(f"{shape} {name}: largest |E - fsum| / bound = {worst:.3e}")


# ---- 3. the same bits however the lattice is held or cut, and whatever is transformed beside a plane --------

def test_in_place_slabs_groups_and_batch_slots_give_the_same_bits(pkg, random_case):
    shape, nranks, groups, f, _, planes, full = random_case
    nz = shape[2]
    p = _params(pkg, shape)

    def check(got, name, z0, n, what):
        assert _same(got[0], full[name][0][z0:z0 + n]), (what, name, "shells")
        assert _same(got[1], full[name][1][z0:z0 + n]), (what, name, "peaks")

    with pkg.Solver(_params(pkg, shape, in_place=1)) as s:
        s.set_fields(f)
        for name in ("uz", "phi"):
            check(s.spectrum(name), name, 0, nz, "in place")
            assert _same(s.spectrum_plane(name, 2), planes[name][2])
    for rank in range(nranks):
        with pkg.Solver(p, rank=rank, nranks=nranks, slab=True) as s:
            z0, nzl = s.z0, s.nz_local
            s.set_fields({n: v[z0:z0 + nzl] for n, v in f.items()})
            for name in ("uz", "phi"):
                check(s.spectrum(name), name, z0, nzl, ("slab", rank))
            # chosen planes: its own rows, +0.0 and (0, 0, 0.0) for the others
            sh, pk = s.spectrum("uz", list(range(nz)))
            own = np.zeros(nz, dtype=bool)
            own[z0:z0 + nzl] = True
            assert _same(sh[own], full["uz"][0][own]) and _same(pk[own], full["uz"][1][own])
            assert _same(sh[~own], np.zeros_like(sh[~own])) and _same(pk[~own], np.zeros_like(pk[~own]))
            other = (z0 + nzl) % nz
            with pytest.raises(pkg.EkpnpError):
                s.spectrum_plane("uz", other)
    for nslabs in groups:
        with pkg.Group(p, nslabs, devices=[0] * nslabs) as g:
            g.set_fields(f)
            for name in ("uz", "phi"):
                check(g.spectrum(name), name, 0, nz, ("group", nslabs))
            got = g.spectrum("uz", [1, nz // 2, nz - 2])
            for k, z in enumerate([1, nz // 2, nz - 2]):
                assert _same(got[0][k], full["uz"][0][z]) and _same(got[1][k], full["uz"][1][z])
            assert _same(g.spectrum_plane("phi", nz - 2), planes["phi"][nz - 2])
    # slot independence: a plane's bits do not depend on which slot of the batch it sits in or on what sits beside it
    with pkg.Solver(p) as s:
        s.set_fields(f)
        for name in ("uz", "phi"):
            for z in range(nz):
                check(s.spectrum(name, [z]), name, z, 1, ("one by one", z))
            for first in (0, 1):
                for z in range(first, nz - 1, 2):
                    check(s.spectrum(name, [z, z + 1]), name, z, 2, ("pairs", z))
            check(s.spectrum(name, list(range(nz))), name, 0, nz, "all chosen")
            check(s.spectrum(name, list(range(3, nz))), name, 3, nz - 3, "from plane 3 on")


def test_sixteen_at_a_time_against_all_planes(pkg):
    """R has 17 planes: all of them are a batch of sixteen and a short one; sixteen chosen ones put every plane into another slot"""
    nx, ny, nz = R
    f = _random_fields(pkg, (nz, ny, nx), 7)
    with pkg.Solver(_params(pkg, R)) as s:
        s.set_fields(f)
        sh, pk = s.spectrum("uz")
        assert sh.shape[0] == nz and pk.shape == (nz, 3)
        for first in (0, 1):
            got = s.spectrum("uz", list(range(first, first + 16)))
            assert _same(got[0], sh[first:first + 16]) and _same(got[1], pk[first:first + 16]), first
        one = s.spectrum("uz", [nz - 1])
        assert _same(one[0][0], sh[nz - 1]) and _same(one[1][0], pk[nz - 1])


# ---- 4. closed loop: seed a pattern, find it -----------------------------------------------------------------

def test_a_seeded_pattern_is_the_peak(pkg):
    nx, ny, nz = W
    A = 1e-3
    with pkg.Solver(_params(pkg, W)) as s:
        s.set_field("uz", np.zeros(s.shape))
        s.seed(pkg.seed_spec(fields=("uz",), pattern="squares", modes=(2, 3), amplitude=A, noise=0.0, relative=False, seed=1))
        v = s.get_field("uz")
        shell_of, count = s.spectrum_shells()
        shells, peaks = s.spectrum("uz")
    nshell = len(count)
    assert shells.shape == (nz, nshell)
    home = shell_of[3, 2]
    assert home == shell_of[ny - 3, 2]  # (2, 3) and (2, -3) lie on the same shell
    for z in range(1, nz - 1):
        env = math.sin(math.pi * z / (nz - 1))
        u = _u(v[z])
        want = 2.0 * (A * env * nx * ny / 4.0) ** 2  # cos a cos b = (cos(a + b) + cos(a - b)) / 2, and w = 2
        m, n, P = peaks[z]
        assert (m, n) in ((2.0, 3.0), (2.0, -3.0)), (z, m, n)
        assert abs(P - want) <= 4.0 * u, (z, P, want, u)
        assert want > 1e6 * u  # (the check has teeth)
        rest = math.fsum(shells[z].tolist()) - shells[z, home]
        assert abs(rest) <= 4.0 * u * nshell, (z, rest, u)
    for z in (0, nz - 1):  # the plates are never seeded: a plane of zeros has no peak
        assert (v[z] == 0.0).all()
        assert _same(shells[z], np.zeros(nshell)) and _same(peaks[z], np.zeros(3))


# ---- 5. NaN ------------------------------------------------------------------------------------------------

def test_a_nan_node_spoils_its_own_plane_only(pkg, random_case):
    shape, _, _, f, (_, count), _, full = random_case
    nz = shape[2]
    v = f["uz"].copy()
    v[3, 5, 7] = np.nan
    with pkg.Solver(_params(pkg, shape)) as s:
        s.set_fields(f)
        s.set_field("uz", v)
        shells, peaks = s.spectrum("uz")
        P = s.spectrum_plane("uz", 3)
    assert np.isnan(P).all()
    assert np.isnan(shells[3][count > 0]).all() and (shells[3][count == 0] == 0.0).all()
    assert _same(peaks[3], np.zeros(3))
    keep = np.arange(nz) != 3
    assert _same(shells[keep], full["uz"][0][keep]) and _same(peaks[keep], full["uz"][1][keep])


# ---- 6. the ring -------------------------------------------------------------------------------------------

SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)
PLANES = [1, 8, 15]


def _seeded_start(pkg, s, **knobs):
    for k, v in knobs.items():
        s.tune(k, v)
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


def _ring_against_twin(pkg, a, b, field, stride, mirror=False):
    """six step / record pairs on a with a ring of four rows; the twin b steps alongside (mirror: is handed a's field values
    instead) and takes the synchronous spectrum each time"""
    assert a.spectrum_count() == (0, 0)
    a.spectrum_arm(field, PLANES, capacity=4)
    want = []
    for k in range(1, 7):
        a.step(stride)
        a.spectrum_record(k * stride, a.t)
        if mirror:
            b.set_field(field, a.get_field(field))
        else:
            b.step(stride)
        want.append((k * stride, a.t if mirror else b.t, *b.spectrum(field, PLANES)))
    assert a.spectrum_count() == (6, 2)
    steps, times, shells, peaks = a.spectrum_read()
    nshell = want[0][2].shape[1]
    assert shells.shape == (4, len(PLANES), nshell) and peaks.shape == (4, len(PLANES), 3)
    assert steps.tolist() == [w[0] for w in want[2:]] and times.tolist() == [w[1] for w in want[2:]]
    for k, w in enumerate(want[2:]):
        assert _same(shells[k], w[2]), (field, w[0], "shells")
        assert _same(peaks[k], w[3]), (field, w[0], "peaks")
    assert np.isfinite(shells).all() and (shells[:, :, 0] > 0.0).all() and (shells[-1] != shells[0]).any()
    # read: oldest first, range checked
    s1, _, sh1, pk1 = a.spectrum_read(1, 2)
    assert s1.tolist() == steps[1:3].tolist() and _same(sh1, shells[1:3]) and _same(pk1, peaks[1:3])
    with pytest.raises(pkg.EkpnpError):
        a.spectrum_read(2, 3)
    with pytest.raises(pkg.EkpnpError):
        a.spectrum_read(-1, 1)
    # disarmed: the rows stay readable, record is refused; armed again: an empty ring
    a.spectrum_disarm()
    assert _same(a.spectrum_read()[2], shells)
    with pytest.raises(pkg.EkpnpError):
        a.spectrum_record(7, 0.0)
    with pytest.raises(pkg.EkpnpError):
        a.spectrum_arm(field, None, capacity=3)  # a time series needs chosen planes
    a.spectrum_arm(field, PLANES[:2], capacity=3)
    assert a.spectrum_count() == (0, 0) and a.spectrum_read()[2].shape == (0, 2, nshell)


@pytest.mark.parametrize("field, stride, batch", [("uz", 1, 0), ("c", 1, 0), ("uz", 2, 1), ("phi", 1, 0)])
def test_ring_rows_equal_a_twins_synchronous_spectra(pkg, field, stride, batch):
    with pkg.Solver(_params(pkg, R)) as a, pkg.Solver(_params(pkg, R)) as b:
        _seeded_start(pkg, a, batch_moments=batch)
        _seeded_start(pkg, b)
        _ring_against_twin(pkg, a, b, field, stride)


def test_ring_on_a_group_equals_a_single_context(pkg):
    """A group's steps differ from a single context's in the last bits (the slabs' z solve adds in another order:
    tests/test_group_gpu.py holds the two to 1e-11 .. 1e-7), so a single context that steps alongside does not hold the group's
    field.  The single-context twin is therefore handed the group's field values after every step - and then its rows are the
    group's bit for bit; a group twin that steps alongside is held to the same."""
    p = _params(pkg, R)
    with pkg.Group(p, 2, devices=[0, 0]) as a, pkg.Solver(p) as b:
        _seeded_start(pkg, a)
        _ring_against_twin(pkg, a, b, "uz", 1, mirror=True)
    with pkg.Group(p, 2, devices=[0, 0]) as a, pkg.Group(p, 2, devices=[0, 0]) as b:
        _seeded_start(pkg, a)
        _seeded_start(pkg, b)
        _ring_against_twin(pkg, a, b, "uz", 1)


# ---- 7. leaves the run alone -------------------------------------------------------------------------------

def test_tracking_leaves_the_step_graph_and_the_run_alone(pkg):
    with pkg.Solver(_params(pkg, R)) as a, pkg.Solver(_params(pkg, R)) as b:
        _seeded_start(pkg, a)
        _seeded_start(pkg, b)
        a.step(5)
        b.step(5)
        assert a.graph_state() == 1
        bytes_before = a.device_bytes()
        a.spectrum_arm("uz", PLANES, capacity=8)
        assert a.graph_state() == 1 and a.device_bytes() > bytes_before
        a.spectrum_record(5, a.t)
        a.step(4)
        a.spectrum_record(9, a.t)
        a.step(2)
        b.step(4)
        b.step(2)
        assert a.graph_state() == 1 and a.spectrum_count() == (2, 0)
        fa, fb = a.fields(), b.fields()
        for n in pkg.FIELDS:
            assert _same(fa[n], fb[n]), n
        assert b.device_bytes() == bytes_before  # a context that never calls the new entry points allocates nothing new


# ---- 8. the driver -----------------------------------------------------------------------------------------

def _run_driver(args, out):
    out.mkdir()
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1", EKPNP_PLACEMENT_TRIES="1")  # the child shares device 0 with this process
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (args, r.stderr[-2000:])
    return out


def _read_spectrum(path):
    lines = open(path).read().splitlines()
    w = lines[0].split()
    assert w[:3] == ["#", "ekpnp", "spectrum"] and w[3:9:2] == ["nx", "ny", "nz"] and w[9] == "field" and w[11] == "planes"
    k = w.index("nshell")
    assert w[k + 2] == "L" and w[k + 4] == "recorded" and w[k + 6] == "dropped" and len(w) == k + 8
    hdr = dict(nx=int(w[4]), ny=int(w[6]), nz=int(w[8]), field=w[10], planes=[int(x) for x in w[12:k]], nshell=int(w[k + 1]), L=float(w[k + 3]),
               recorded=int(w[k + 5]), dropped=int(w[k + 7]))
    cols = lines[1].split()
    assert cols == ["#", "step", "time", "z", "peak_m", "peak_n", "peak_P"] + [f"E_{s}" for s in range(hdr["nshell"])]
    rows = [ln.split() for ln in lines[2:]]
    assert all(len(r) == len(cols) - 1 for r in rows)
    assert all(" ".join(r) == ln for r, ln in zip(rows, lines[2:]))  # single spaces
    return hdr, rows


GEO = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "6", "--seed-pattern", "squares", "--seed-modes", "1,1"]


def test_driver_writes_the_spectrum_file(pkg, tmp_path):
    assert os.path.exists(EXE), "ekpnp_main not built"
    track = ["--spectrum-every", "1", "--spectrum-field", "c"]
    plain = _run_driver(GEO, tmp_path / "plain")
    loop = _run_driver([*GEO, *track], tmp_path / "loop")
    batch = _run_driver([*GEO, *track, "--batch", "1"], tmp_path / "batch")
    p = pkg.default_params(40, 12, 17)
    hdr, rows = _read_spectrum(loop / "spectrum.dat")
    assert hdr == dict(nx=40, ny=12, nz=17, field="c", planes=[8], nshell=len(pkg.spectrum_shells(p)[1]), L=max(p.Lx, p.Ly), recorded=6, dropped=0)
    assert len(rows) == 6 and [int(r[0]) for r in rows] == [1, 2, 3, 4, 5, 6] and all(int(r[2]) == 8 for r in rows)
    assert np.isfinite(np.array([[float(x) for x in r] for r in rows])).all()
    for r in rows:
        assert (int(r[3]), int(r[4])) in ((1, 1), (1, -1)), r[:6]
        assert float(r[5]) > 0.0
    assert (loop / "spectrum.dat").read_bytes() == (batch / "spectrum.dat").read_bytes()
    assert not (plain / "spectrum.dat").exists()
    for f in ("data.dat", "umax.dat", "data_end.dat"):
        a = (plain / f).read_bytes()
        assert len(a) > 0 and a == (loop / f).read_bytes() and a == (batch / f).read_bytes(), f
