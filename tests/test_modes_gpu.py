"""GPU tests of the projection onto chosen x-y modes and its time series (csrc/modes.hip; include/ekpnp.h: ekpnp_mode_amplitudes,
ekpnp_modes_* and the ekpnp_group_* spellings; `ekpnp_main --modes-every N`).

Per plane and mode a = sum v cos(theta), b = sum v sin(theta).  They are held against math.fsum of the double products with a
bound that is derived, not measured: |gpu - exact| <= (nx*ny + 16) * 2**-53 * fsum(|v|), the first-order bound for ANY order of
nx*ny additions plus a few roundings per term (|cos|, |sin| <= 1).  On the inputs used here the kernel stays below
5e-5 of that bound (the test prints the figure), so the reference alone is nowhere near it.  Everything that can be exact is held
exactly: integer fields, the bits across buffer modes and decompositions, the ring against a twin's synchronous values."""
import math
import os
import subprocess

import numpy as np
import pytest

from _observer_pairs import TRACK, energies

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
R = (40, 12, 17)
W = (70, 66, 13)
V = (128, 36, 9)   # rows of a multiple of 64 nodes (the kernel then loads a row's table entry once per wavefront), two workgroups per plane, slabs of 4 + 5
MODES = [(0, 0), (1, 0), (0, 1), (35, 0), (3, -2), (35, 33), (1, 33), (17, -32)]
CASES = {"W": (W, MODES, 3, (2, 3)), "V": (V, [(0, 0), (1, 0), (0, 1), (64, 0), (3, -2), (64, 18), (1, 18), (17, -17)], 2, (2,))}


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
    return {n: scale.get(n, 1e-3) * rng.uniform(-1.0, 1.0, size=shape_zyx) for n in pkg.FIELDS}


def _phase(nx, ny, m, n):
    """cos(theta), sin(theta) on the plane with the phase reduced exactly in integers: theta = 2 pi k / (nx ny)"""
    x, y = np.arange(nx)[None, :], np.arange(ny)[:, None]
    k = (m * x * ny + n * y * nx) % (nx * ny)
    th = 2.0 * np.pi * k.astype(np.float64) / float(nx * ny)
    return np.cos(th), np.sin(th)


_energies = energies   # [nmodes] from [nmodes][planes][2] in the prescribed order (tests/_observer_pairs.py, shared with the pair tests)


@pytest.fixture(scope="module", params=list(CASES))
def random_case(pkg, request):
    """random fields of W or V and the (a, b) of uz and phi on a two-buffer context (computed once, never modified)"""
    shape, modes, nranks, groups = CASES[request.param]
    f = _random_fields(pkg, (shape[2], shape[1], shape[0]), 31)
    with pkg.Solver(_params(pkg, shape)) as s:
        s.set_fields(f)
        ab = {name: s.mode_amplitudes(name, modes) for name in ("uz", "phi")}
    return shape, modes, nranks, groups, f, ab


# ---- 1. against exact sums ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["uz", "phi"])
def test_amplitudes_against_fsum_of_the_double_products(pkg, random_case, name):
    shape, modes, _, _, f, ab = random_case
    nx, ny, nz = shape
    got = ab[name]
    assert got.shape == (len(modes), nz, 2)
    worst = 0.0
    for j, (m, n) in enumerate(modes):
        ct, st = _phase(nx, ny, m, n)
        for z in range(nz):
            v = f[name][z]
            bound = (nx * ny + 16) * 2.0 ** -53 * math.fsum(np.abs(v).ravel().tolist())
            for k, w in enumerate((ct, st)):
                exact = math.fsum((v * w).ravel().tolist())
                err = abs(got[j, z, k] - exact)
                worst = max(worst, err / bound)
                assert err <= bound, (name, (m, n), z, "ab"[k], got[j, z, k], exact, err, bound)
    print(f"{shape} {name}: largest |gpu - exact| / bound = {worst:.3e}")


@pytest.mark.parametrize("shape", [W, V])
def test_integer_fields_give_exact_sums(pkg, shape):
    nx, ny, nz = shape
    rng = np.random.default_rng(3)
    v = rng.integers(-1000, 1001, size=(nz, ny, nx)).astype(np.float64)
    with pkg.Solver(_params(pkg, shape)) as s:
        s.set_field("T", v)
        ab = s.mode_amplitudes("T", [(0, 0), (nx // 2, 0)])
    sign = np.where(np.arange(nx) % 2 == 0, 1.0, -1.0)[None, None, :]
    assert np.array_equal(ab[0, :, 0], v.sum(axis=(1, 2)))           # |sum| < 2**53: exact in any order
    assert (ab[0, :, 1] == 0.0).all()
    assert np.array_equal(ab[1, :, 0], (v * sign).sum(axis=(1, 2)))  # cos(pi x) = +-1 exactly


# ---- 2. the same bits however the lattice is held or cut ------------------------------------------------

def test_in_place_slabs_and_groups_give_the_same_bits(pkg, random_case):
    shape, MODES, nranks, groups, f, ab = random_case
    p = _params(pkg, shape)
    with pkg.Solver(_params(pkg, shape, in_place=1)) as s:
        s.set_fields(f)
        for name in ("uz", "phi"):
            assert _same(s.mode_amplitudes(name, MODES), ab[name]), ("in place", name)
    for rank in range(nranks):
        with pkg.Solver(p, rank=rank, nranks=nranks, slab=True) as s:
            z0, nzl = s.z0, s.nz_local
            s.set_fields({n: v[z0:z0 + nzl] for n, v in f.items()})
            for name in ("uz", "phi"):
                assert _same(s.mode_amplitudes(name, MODES), ab[name][:, z0:z0 + nzl]), ("slab", rank, name)
    for nslabs in groups:
        with pkg.Group(p, nslabs, devices=[0] * nslabs) as g:
            g.set_fields(f)
            for name in ("uz", "phi"):
                assert _same(g.mode_amplitudes(name, MODES), ab[name]), ("group", nslabs, name)
    # a mode's (a, b) do not depend on what is projected beside it (1, 2, 4, 8 and 16 modes take different kernels)
    with pkg.Solver(p) as s:
        s.set_fields(f)
        for k in (1, 2, 3, 5):
            assert _same(s.mode_amplitudes("uz", MODES[2:2 + k]), ab["uz"][2:2 + k]), k
        twice = s.mode_amplitudes("uz", MODES + MODES)
        assert _same(twice[:8], ab["uz"]) and _same(twice[8:], ab["uz"])


# ---- 3. closed loop: seed a mode, read it back -------------------------------------------------------------

def test_a_seeded_mode_is_read_back(pkg):
    nx, ny, nz = W
    A = 1e-3
    modes = [(2, 3), (2, -3), (2, 0), (0, 0)]
    with pkg.Solver(_params(pkg, W)) as s:
        s.set_field("uz", np.zeros(s.shape))
        s.seed(pkg.seed_spec(fields=("uz",), pattern="squares", modes=(2, 3), amplitude=A, noise=0.0, relative=False, seed=1))
        v = s.get_field("uz")
        ab = s.mode_amplitudes("uz", modes)
    assert (v[0] == 0.0).all() and (v[-1] == 0.0).all()
    for z in range(1, nz - 1):
        env = math.sin(math.pi * z / (nz - 1))
        bound = (nx * ny + 16) * 2.0 ** -53 * math.fsum(np.abs(v[z]).ravel().tolist())
        assert bound > 0.0
        want = A * env * nx * ny / 4.0
        for j in (0, 1):  # cos a cos b = (cos(a + b) + cos(a - b)) / 2: half the amplitude in each of the two modes
            assert abs(ab[j, z, 0] - want) <= bound, (modes[j], z, ab[j, z, 0], want, bound)
            assert abs(ab[j, z, 1]) <= bound, (modes[j], z, ab[j, z, 1], bound)
        for j in (2, 3):
            assert abs(ab[j, z, 0]) <= bound and abs(ab[j, z, 1]) <= bound, (modes[j], z, ab[j, z], bound)
        assert want > 1e6 * bound  # (the check has teeth)
    assert (ab[:, 0] == 0.0).all() and (ab[:, -1] == 0.0).all()


# ---- 4. the ring -------------------------------------------------------------------------------------------

SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)


def _seeded_start(pkg, s, **knobs):
    for k, v in knobs.items():
        s.tune(k, v)
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


@pytest.mark.parametrize("field, stride, batch", [("uz", 1, 0), ("c", 1, 0), ("uz", 2, 1), ("phi", 1, 0)])
def test_ring_rows_equal_a_twins_synchronous_amplitudes(pkg, field, stride, batch):
    with pkg.Solver(_params(pkg, R)) as a, pkg.Solver(_params(pkg, R)) as b:
        _seeded_start(pkg, a, batch_moments=batch)
        _seeded_start(pkg, b)
        assert a.modes_count() == (0, 0)
        a.modes_arm(field, TRACK, capacity=4)
        want = []
        for k in range(1, 7):
            a.step(stride)
            a.modes_record(k * stride, a.t)
            b.step(stride)
            want.append((k * stride, b.t, _energies(b.mode_amplitudes(field, TRACK))))
        assert a.modes_count() == (6, 2)
        steps, times, values = a.modes_read()
        assert values.shape == (4, len(TRACK))
        assert steps.tolist() == [w[0] for w in want[2:]] and times.tolist() == [w[1] for w in want[2:]]
        for row, w in zip(values, want[2:]):
            assert _same(row, w[2]), (field, w[0], row, w[2])
        assert (values[:, 0] > 0.0).all() and (values[-1] != values[0]).any()
        # read: oldest first, range checked
        s1, _, v1 = a.modes_read(1, 2)
        assert s1.tolist() == steps[1:3].tolist() and _same(v1, values[1:3])
        with pytest.raises(pkg.EkpnpError):
            a.modes_read(2, 3)
        # disarmed: the rows stay readable, record is refused; armed again: an empty ring
        a.modes_disarm()
        assert _same(a.modes_read()[2], values)
        with pytest.raises(pkg.EkpnpError):
            a.modes_record(7, 0.0)
        a.modes_arm(field, TRACK[:2], capacity=3)
        assert a.modes_count() == (0, 0) and a.modes_read()[2].shape == (0, 2)


def test_ring_on_a_group_adds_the_slabs_in_ascending_order(pkg):
    p = _params(pkg, R)
    with pkg.Group(p, 2, devices=[0, 0]) as a, pkg.Group(p, 2, devices=[0, 0]) as b:
        _seeded_start(pkg, a)
        _seeded_start(pkg, b)
        cut = a.slab_extent(1)[0]
        a.modes_arm("uz", TRACK, capacity=4)
        want = []
        for k in range(1, 7):
            a.step(1)
            a.modes_record(k, a.t)
            b.step(1)
            ab = b.mode_amplitudes("uz", TRACK)
            want.append(_energies(ab[:, :cut]) + _energies(ab[:, cut:]))
        assert a.modes_count() == (6, 2)
        steps, _, values = a.modes_read()
        assert steps.tolist() == [3, 4, 5, 6]
        for row, w in zip(values, want[2:]):
            assert _same(row, w), (row, w)

def test_tracking_leaves_the_step_graph_and_the_run_alone(pkg):
    with pkg.Solver(_params(pkg, R)) as a, pkg.Solver(_params(pkg, R)) as b:
        _seeded_start(pkg, a)
        _seeded_start(pkg, b)
        a.step(5)
        b.step(5)
        assert a.graph_state() == 1
        bytes_before = a.device_bytes()
        a.modes_arm("uz", TRACK, capacity=8)
        assert a.graph_state() == 1 and a.device_bytes() > bytes_before
        a.modes_record(5, a.t)
        a.step(4)
        a.modes_record(9, a.t)
        a.step(2)
        b.step(4)
        b.step(2)
        assert a.graph_state() == 1 and a.modes_count() == (2, 0)
        fa, fb = a.fields(), b.fields()
        for n in pkg.FIELDS:
            assert _same(fa[n], fb[n]), n
        assert b.device_bytes() == bytes_before  # a context that never calls the new entry points allocates nothing new


# ---- 5. the driver -----------------------------------------------------------------------------------------

def _run_driver(args, out):
    out.mkdir()
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1", EKPNP_PLACEMENT_TRIES="1")  # the child shares device 0 with this process
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (args, r.stderr[-2000:])
    return out


def _read_modes(path):
    lines = open(path).read().splitlines()
    w = lines[0].split()
    assert w[:3] == ["#", "ekpnp", "modes"] and w[3:9:2] == ["nx", "ny", "nz"] and w[9] == "field" and w[11] == "recorded" and w[13] == "dropped"
    hdr = dict(nx=int(w[4]), ny=int(w[6]), nz=int(w[8]), field=w[10], recorded=int(w[12]), dropped=int(w[14]))
    cols = lines[1].split()
    assert cols[:3] == ["#", "step", "time"]
    rows = [ln.split() for ln in lines[2:]]
    assert all(len(r) == len(cols) - 1 for r in rows)
    return hdr, cols[3:], [int(r[0]) for r in rows], np.array([[float(x) for x in r[1:]] for r in rows])


GEO = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "6"]


def test_driver_seeds_and_tracks(pkg, tmp_path):
    assert os.path.exists(EXE), "ekpnp_main not built"
    track = ["--modes-every", "1", "--modes-field", "c"]
    seed = ["--seed-pattern", "squares", "--seed-modes", "1,1"]
    loop = _run_driver([*GEO, *seed, *track], tmp_path / "loop")
    batch = _run_driver([*GEO, *seed, *track, "--batch", "1"], tmp_path / "batch")
    unseeded = _run_driver([*GEO, *track], tmp_path / "unseeded")
    hdr, names, steps, rows = _read_modes(loop / "modes.dat")
    assert hdr == dict(nx=40, ny=12, nz=17, field="c", recorded=6, dropped=0)
    assert names == ["E_1_1", "E_1_-1", "E_0_0"] and steps == [1, 2, 3, 4, 5, 6]
    assert np.isfinite(rows).all() and (rows[:, 1:] > 0.0).all()
    assert (loop / "modes.dat").read_bytes() == (batch / "modes.dat").read_bytes()
    for f in ("data.dat", "umax.dat", "data_end.dat"):
        assert (loop / f).read_bytes() == (batch / f).read_bytes(), f
    _, unames, _, urows = _read_modes(unseeded / "modes.dat")
    assert unames == names
    # the unseeded energy is rounding of a uniform plane, of order (nx ny 2**-53)**2 relative: the true ratio is above 1e20
    print(f"E_1_1 of the first row: seeded {rows[0, 1]:.6e}, unseeded {urows[0, 1]:.6e}")
    assert rows[0, 1] >= 1e6 * urows[0, 1] and rows[0, 1] > 0.0


def test_driver_without_the_new_flags_writes_what_it_wrote(pkg, tmp_path):
    """a seed that adds nothing is skipped together with its solve: the files of a run without any new flag, byte for byte"""
    plain = _run_driver(GEO, tmp_path / "plain")
    zero = _run_driver([*GEO, "--seed-pattern", "noise", "--seed-noise", "0"], tmp_path / "zero")
    assert not (plain / "modes.dat").exists() and not (zero / "modes.dat").exists()
    for f in ("data.dat", "umax.dat", "data_end.dat"):
        a = (plain / f).read_bytes()
        assert len(a) > 0 and a == (zero / f).read_bytes(), f
