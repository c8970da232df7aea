"""GPU tests of the tracers' sort by cell (csrc/tracers.hip: k_tracers_sort_*; include/ekpnp.h: ekpnp_tracers_sort, ekpnp_tracers_ids;
`ekpnp_main --tracers-sort-every K`).

ekpnp_tracers_sort_host is the definition (tests/test_tracers_sort_cpu.py holds it against numpy's stable argsort) and its result is
unique, so the device is compared with it EXACTLY: every array on its bit pattern, the ids as integers.  The one toleranced check
is the moments' sums, which are added in slot order: the a-priori bound n * 2^-53 * sum|term| of any order of n additions, as in
tests/test_tracers_gpu.py.  All eight arrays and the ids of a cloud are read through the cloud's own file (ekpnp_tracers_save).

Lattices: W 70 x 66 x 13, O 35 x 33 x 5, R 40 x 12 x 17 of the tracer tests, and T 70 x 66 x 17 with nx*ny*(nz-1) = 73 920 > 65 536: the third
key byte takes two values there and the lost particles give the fourth two, so all four passes see more than one digit.  n = 1 (one
lane), 63 / 64 / 65 (a wavefront and either side), 256, 1000 (a ragged workgroup), 4096 (exactly one run), 4097 (one past it) and
3*4096 + 77 (several runs and a tail)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _tracers_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
SHAPES = {"W": (70, 66, 13), "O": (35, 33, 5), "R": (40, 12, 17), "T": (70, 66, 17)}
NS = (1, 63, 64, 65, 256, 1000, 4096, 4097, 3 * 4096 + 77)
UE = ("ux", "uy", "uz", "Ex", "Ey", "Ez")
ARRAYS = ("x", "y", "z", "x0", "y0", "z0", "wx", "wy")


def _params(pkg, shape):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    return p


@pytest.fixture(scope="module")
def inputs(pkg):
    """per lattice: (u, E) random fields; made once, never modified"""
    out = {}
    for k, s in SHAPES.items():
        u, E = T.random_fields(s, 181 + len(out), T.U_SCALE, T.E_SCALE)
        for a in (*u, *E):
            a.setflags(write=False)
        out[k] = (u, E)
    return out


def _put_fields(s, u, E):
    for name, a in zip(UE, (*u, *E)):
        s.set_field(name, a)


def _parse(raw):
    """the cloud's file: ({x, y, z, x0, y0, z0, wx, wy}, ids or None, reserved)"""
    assert raw[:8] == b"EKPNPTR1"
    reserved = int(np.frombuffer(raw[20:24], dtype="<i4")[0])
    n = int(np.frombuffer(raw[24:32], dtype="<i8")[0])
    assert len(raw) == 48 + (60 if reserved == 1 else 56) * n, (len(raw), reserved, n)
    d = np.frombuffer(raw[48:48 + 48 * n], dtype="<f8").reshape(6, n)
    w = np.frombuffer(raw[48 + 48 * n:48 + 56 * n], dtype="<i4").reshape(2, n)
    cloud = dict(zip(ARRAYS, [*d, *w]))
    ids = np.frombuffer(raw[48 + 56 * n:], dtype="<i4") if reserved == 1 else None
    return cloud, ids, reserved


def _dump(s, path):
    s.tracers_save(str(path), time=0.5)
    return _parse(open(path, "rb").read())


def _same_array(got, want):
    if got.dtype == np.float64:
        return T.same(got, want)
    return got.dtype == want.dtype and np.array_equal(got, want)


def _assert_permuted(after, before, perm, what):
    for name in ARRAYS:
        assert _same_array(after[name], before[name][perm]), (what, name)


def _clouds(shape, n, seed):
    """the clouds of the issue but the advanced one: name -> (x, y, z)"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    nodes = nx * ny * (nz - 1)
    k = (n - 1 - np.arange(n)) % nodes   # descending node index: memory order reversed
    nan = np.full(n, np.nan)
    return {
        "special": T.special_cloud(shape, n, seed),
        "one node": (3.0 + rng.uniform(0, 1, n), 5.0 + rng.uniform(0, 1, n), 2.0 + rng.uniform(0, 1, n)),
        "all lost": (nan, nan, nan),
        "reversed": ((k % nx) + 0.25, ((k // nx) % ny) + 0.5, (k // (nx * ny)) + 0.75),
    }


# ---- 1. the device equals the definition -----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["W", "O", "R", "T"])
def test_device_sort_equals_sort_host(pkg, inputs, shape, tmp_path):
    u, E = inputs[shape]
    p = _params(pkg, SHAPES[shape])
    path = tmp_path / "cloud.bin"
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        for n in NS:
            clouds = _clouds(SHAPES[shape], n, 300 + n)
            for name, (x, y, z) in clouds.items():
                s.tracers_set(x, y, z)
                before, ids, reserved = _dump(s, path)
                assert ids is None and reserved == 0
                perm = pkg.tracers_sort_host(p, x, y, z)
                s.tracers_sort()
                after, ids, reserved = _dump(s, path)
                assert reserved == 1 and np.array_equal(ids, perm) and np.array_equal(s.tracers_ids(), perm), (shape, n, name)
                _assert_permuted(after, before, perm, (shape, n, name))
                if name == "one node" or name == "all lost":
                    assert np.array_equal(perm, np.arange(n))
                if name == "reversed" and n <= 4096:
                    assert np.array_equal(perm, np.arange(n - 1, -1, -1))
            # a cloud already advanced with a mobility: wx, wy are non-zero and the start differs from the position - all eight arrays differ
            x, y, z = clouds["special"]
            s.tracers_set(x, y, z)
            s.tracers_advance(T.substep(p), nsub=7, mu=T.MU)
            before, _, _ = _dump(s, path)
            if n >= 1000:
                assert before["wx"].any() and before["wy"].any() and not T.same(before["x"], before["x0"]) and np.isnan(before["x"]).any()
            perm = pkg.tracers_sort_host(p, before["x"], before["y"], before["z"])
            s.tracers_sort()
            after, ids, _ = _dump(s, path)
            assert np.array_equal(ids, perm), (shape, n, "advanced")
            _assert_permuted(after, before, perm, (shape, n, "advanced"))
            if n >= 1000:
                keys = pkg.tracers_sort_key(p, after["x"], after["y"], after["z"]).astype(np.int64)
                assert (np.diff(keys) >= 0).all() and keys[-1] == pkg.TRACERS_KEY_LOST
                if shape == "T":   # every pass saw more than one digit
                    assert all(len(set((keys >> (8 * b)) & 255)) > 1 for b in range(4))


# ---- 2. idempotent, and sorts compose --------------------------------------------------------------------------------

def test_a_second_sort_changes_nothing_and_sorts_compose(pkg, inputs, tmp_path):
    u, E = inputs["T"]
    p = _params(pkg, SHAPES["T"])
    path = tmp_path / "cloud.bin"
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        for n in (65, 4097, 3 * 4096 + 77):
            x, y, z = T.special_cloud(SHAPES["T"], n, 400 + n)
            s.tracers_set(x, y, z)
            s.tracers_advance(T.substep(p), nsub=3, mu=T.MU)
            s.tracers_sort()
            first, ids1, _ = _dump(s, path)
            s.tracers_sort()   # fully sorted input: a stable sort leaves every slot where it is
            second, ids2, _ = _dump(s, path)
            assert np.array_equal(ids1, ids2)
            _assert_permuted(second, first, np.arange(n), n)
            s.tracers_advance(T.substep(p), nsub=2, mu=T.MU)
            moved, _, _ = _dump(s, path)
            perm2 = pkg.tracers_sort_host(p, moved["x"], moved["y"], moved["z"])
            assert n < 1000 or not np.array_equal(perm2, np.arange(n))
            s.tracers_sort()
            third, ids3, _ = _dump(s, path)
            assert np.array_equal(ids3, ids1[perm2]) and np.array_equal(s.tracers_ids(), ids1[perm2])
            _assert_permuted(third, moved, perm2, n)


# ---- 3. sorting changes no trajectory --------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["W", "O"])
def test_sorting_changes_no_trajectory(pkg, inputs, shape):
    u, E = inputs[shape]
    p = _params(pkg, SHAPES[shape])
    n = 4097
    x, y, z = T.special_cloud(SHAPES[shape], n, 500)
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        for mu in (0.0, T.MU):
            for nsub in (1, 7):
                s.tracers_set(x, y, z)
                s.tracers_advance(T.substep(p), nsub=nsub, mu=mu)
                s.tracers_advance(T.substep(p), nsub=nsub, mu=mu)
                want = s.tracers_get()
                s.tracers_set(x, y, z)
                s.tracers_sort()
                s.tracers_advance(T.substep(p), nsub=nsub, mu=mu)
                s.tracers_sort()
                s.tracers_advance(T.substep(p), nsub=nsub, mu=mu)
                assert not np.array_equal(s.tracers_ids(), np.arange(n))
                got = s.tracers_get(by_id=True)
                for k, name in enumerate(("x", "y", "z")):
                    assert T.same(got[k], want[k]), (shape, mu, nsub, name)
                assert np.array_equal(np.isnan(got[0]), np.isnan(want[0])) and np.isnan(want[0]).any()
                assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
                assert want[3].any()
                raw = s.tracers_get()
                assert not T.same(raw[0], want[0])   # the slots really moved


# ---- 4. around it: cell counts and moments ---------------------------------------------------------------------------

def test_cell_counts_and_moments_after_a_sort(pkg, inputs, tmp_path):
    shape = SHAPES["W"]
    u, E = inputs["W"]
    p = _params(pkg, shape)
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        for n in (1, 1000, 4097):
            x, y, z = T.special_cloud(shape, n, 600 + n)
            s.tracers_set(x, y, z)
            s.tracers_advance(T.substep(p), nsub=7, mu=T.MU)
            counts = [s.tracers_cell_counts(c) for c in ((4, 3, 2), (70, 66, 12))]
            m0 = s.tracers_moments()
            s.tracers_sort()
            for c, (want, lost) in zip(((4, 3, 2), (70, 66, 12)), counts):
                got, glost = s.tracers_cell_counts(c)
                assert np.array_equal(got, want) and glost == lost, (n, c)
            m1 = s.tracers_moments()
            for q in (0, 1, 10, 11):
                assert m1[q] == m0[q], (n, pkg.TRACER_MOMENTS[q])
            c, _, _ = _dump(s, tmp_path / "cloud.bin")
            alive = ~np.isnan(c["x"])
            dx = (c["x"][alive] - c["x0"][alive]) + c["wx"][alive].astype(np.float64) * float(shape[0])
            dy = (c["y"][alive] - c["y0"][alive]) + c["wy"][alive].astype(np.float64) * float(shape[1])
            dz = c["z"][alive] - c["z0"][alive]
            za = c["z"][alive]
            assert m1[0] == alive.sum() and m1[1] == n - alive.sum()
            for k, t in enumerate([dx, dy, dz, dx * dx, dy * dy, dz * dz, za, za * za]):
                tol = n * 2.0 ** -53 * np.abs(t).sum()
                for m, when in ((m0, "before"), (m1, "after")):
                    d = abs(m[2 + k] - math.fsum(t))
                    print(f"n {n} {pkg.TRACER_MOMENTS[2 + k]} {when} the sort: {d:.3e} (tol {tol:.3e})")
                    assert d <= tol, (n, pkg.TRACER_MOMENTS[2 + k], when, d, tol)


# ---- 5. the file -----------------------------------------------------------------------------------------------------

def test_the_file_carries_the_ids_of_a_sorted_cloud(pkg, inputs, tmp_path):
    shape = SHAPES["W"]
    u, E = inputs["W"]
    p = _params(pkg, shape)
    h = T.substep(p)
    n = 4097
    x, y, z = T.special_cloud(shape, n, 700)
    path = str(tmp_path / "sorted.bin")
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        _put_fields(a, u, E)
        _put_fields(b, u, E)
        a.tracers_set(x, y, z)
        a.tracers_advance(h, nsub=3, mu=T.MU)
        a.tracers_save(str(tmp_path / "plain.bin"), time=0.25)
        plain = open(tmp_path / "plain.bin", "rb").read()
        assert len(plain) == 48 + 56 * n and np.frombuffer(plain[8:24], dtype="<i4").tolist() == [70, 66, 13, 0]
        a.tracers_sort()
        a.tracers_save(path, time=0.125)
        raw = open(path, "rb").read()
        assert len(raw) == 48 + 60 * n and np.frombuffer(raw[8:24], dtype="<i4").tolist() == [70, 66, 13, 1]
        assert np.frombuffer(raw[24:32], dtype="<i8")[0] == n and np.frombuffer(raw[32:40], dtype="<f8")[0] == 0.125
        ids = a.tracers_ids()
        assert np.array_equal(np.frombuffer(raw[48 + 56 * n:], dtype="<i4"), ids) and np.array_equal(np.sort(ids), np.arange(n))
        # load into a fresh context and continue: as if it had not stopped, ids included
        bytes0 = b.device_bytes()
        assert b.tracers_load(path) == 0.125 and b.tracers_size == n
        assert b.device_bytes() == bytes0 + 56 * n + 2 * 96 + 96 + 4 * n   # the cloud, its partials (2 runs) and result, and the ids
        assert np.array_equal(b.tracers_ids(), ids)
        for s in (a, b):
            s.tracers_advance(h, nsub=2, mu=T.MU)
            s.tracers_sort()
            s.tracers_advance(h, nsub=2, mu=T.MU)
        ca, ia, _ = _dump(a, tmp_path / "a.bin")
        cb, ib, _ = _dump(b, tmp_path / "b.bin")
        assert np.array_equal(ia, ib) and not np.array_equal(ia, ids)
        _assert_permuted(cb, ca, np.arange(n), "continued")
        want = pkg.tracers_advance_host(p, u, x, y, z, E=E, mu=T.MU, h=h, nsub=7)
        got = b.tracers_get(by_id=True)
        assert all(T.same(got[k], want[k]) for k in range(3)) and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
        # refusals: a duplicate id (the message names the slot), an id out of range, an unknown reserved value, a short file
        bad = bytearray(raw)
        bad[48 + 56 * n + 4 * 100:48 + 56 * n + 4 * 101] = np.int32(ids[7]).tobytes()
        open(tmp_path / "dup.bin", "wb").write(bytes(bad))
        bad = bytearray(raw)
        bad[48 + 56 * n + 4 * 33:48 + 56 * n + 4 * 34] = np.int32(n).tobytes()
        open(tmp_path / "range.bin", "wb").write(bytes(bad))
        bad = bytearray(raw)
        bad[20:24] = np.int32(2).tobytes()
        open(tmp_path / "reserved.bin", "wb").write(bytes(bad))
        open(tmp_path / "short.bin", "wb").write(raw[:-4])
        for name, msg in (("dup.bin", "slot 100 "), ("range.bin", "slot 33 "), ("reserved.bin", "reserved = 2"), ("short.bin", "shorter")):
            with pytest.raises(pkg.EkpnpError) as e:
                b.tracers_load(str(tmp_path / name))
            assert msg in str(e.value) and "status 1" in str(e.value), name
        assert np.array_equal(b.tracers_ids(), ib)   # a refused load leaves the cloud and its ids alone
        # seed, set and a load of a file without ids reset the ids to the identity, and such a cloud writes the old file again
        one = np.arange(n)
        assert b.tracers_load(str(tmp_path / "plain.bin")) == 0.25 and np.array_equal(b.tracers_ids(), one)
        assert _dump(b, tmp_path / "c.bin")[2] == 0
        b.tracers_sort()
        assert not np.array_equal(b.tracers_ids(), one)
        b.tracers_set(x, y, z)
        assert np.array_equal(b.tracers_ids(), one) and _dump(b, tmp_path / "c.bin")[2] == 0
        b.tracers_sort()
        b.tracers_seed(n=n, seed=3)
        assert np.array_equal(b.tracers_ids(), one) and _dump(b, tmp_path / "c.bin")[2] == 0
        b.tracers_sort()
        b.tracers_seed(n=1000, seed=3)   # another size: the id array of the old cloud is gone with it
        assert np.array_equal(b.tracers_ids(), np.arange(1000))


# ---- 6. the run is left alone ----------------------------------------------------------------------------------------

SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)


def _seeded_start(pkg, s):
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


def test_device_bytes_and_the_step_graph(pkg):
    p = _params(pkg, SHAPES["R"])
    n = 3 * 4096 + 77
    cloud = 56 * n + (4 + 1) * 12 * 8          # four runs of 4096 particles of partial moments and the result
    scratch = 16 * n + (256 * 4 + 1) * 4       # two item buffers, the digit table of four runs and its one chunk sum
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        _seeded_start(pkg, a)
        _seeded_start(pkg, b)
        a.step(5)
        b.step(5)
        state = a.graph_state()
        before = a.device_bytes()
        with pytest.raises(pkg.EkpnpError) as e:
            a.tracers_sort()
        assert "tracers: no cloud" in str(e.value) and "status 1" in str(e.value)
        with pytest.raises(pkg.EkpnpError) as e:
            a.tracers_ids()
        assert "tracers: no cloud" in str(e.value)
        for s in (a, b):
            s.tracers_seed(n=n, seed=1)
        assert a.device_bytes() == before + cloud and b.device_bytes() == before + cloud   # today's formula
        assert np.array_equal(b.tracers_ids(), np.arange(n)) and b.device_bytes() == before + cloud   # asking for ids allocates nothing
        for k in range(4):
            a.step(1)
            b.step(1)
            a.tracers_sort()
            for s in (a, b):
                s.tracers_advance(p.dt, nsub=2, mu=1e-8 if k % 2 else 0.0)
            assert a.device_bytes() == before + cloud + scratch + 4 * n and b.device_bytes() == before + cloud
        assert a.graph_state() == state and b.graph_state() == state
        fa, fb = a.fields(), b.fields()
        for name in pkg.FIELDS:
            assert np.array_equal(T.bits(fa[name]), T.bits(fb[name])), name
        ga, gb = a.tracers_get(by_id=True), b.tracers_get()
        assert all(T.same(ga[k], gb[k]) for k in range(3))
        a.tracers_release()
        assert a.device_bytes() == before   # release gives the scratch and the ids back too


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as G
pkg = G.load_package()
p = pkg.default_params(40, 12, 17)
with pkg.Solver(p) as s:
    s.tracers_seed(n=5000, seed=1)
    s.tracers_advance(1e-9, nsub=2)
    s.tracers_moments(); s.tracers_cell_counts((4, 3, 2)); s.tracers_ids(); s.tracers_save(sys.argv[1])
    print("PLAIN OK")
    try:
        s.tracers_sort()
        print("SORT OK")
    except pkg.EkpnpError as e:
        print("ERR", e)
''' % ROOT


@pytest.mark.parametrize("kernel", ["k_tracers_sort_keys", "k_tracers_sort_scatter", "k_tracers_sort_gather"])
def test_a_context_that_never_sorts_launches_no_sort_kernel(kernel, tmp_path):
    """the library's launch-failure knob (read once per process, hence a child) fails the named kernel's first launch: everything
    a cloud did before this change goes through, and the sort reports that kernel by name"""
    env = dict(os.environ, EKPNP_INJECT_LAUNCH_FAILURE=kernel)
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "c.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PLAIN OK" in r.stdout and "ERR" in r.stdout and f"kernel {kernel}:" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert os.path.getsize(tmp_path / "c.bin") == 48 + 56 * 5000


def test_slab_contexts_are_refused(pkg):
    p = _params(pkg, SHAPES["W"])
    msg = "tracers: slab contexts are not supported"
    for rank, nranks in ((0, 1), (1, 3)):
        with pkg.Solver(p, rank=rank, nranks=nranks, slab=True) as s:
            for k, call in enumerate((lambda: s.tracers_sort(), lambda: s.tracers_ids(), lambda: s.tracers_get(by_id=True))):
                with pytest.raises(pkg.EkpnpError) as e:
                    call()
                assert "status 1" in str(e.value) and msg in str(e.value), k


# ---- 7. the driver ---------------------------------------------------------------------------------------------------

def _run_driver(args, out):
    out.mkdir()
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1", EKPNP_PLACEMENT_TRIES="1")  # the child shares device 0 with this process
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (args, r.stderr[-2000:])
    return out


def test_driver_sorts_every_kth_advance_and_changes_no_trajectory(pkg, tmp_path):
    assert os.path.exists(EXE), "ekpnp_main not built"
    geo = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "12", "--seed-pattern", "squares", "--seed-modes", "1,1"]
    n = 4097
    flags = ["--tracers", str(n), "--tracers-every", "2", "--tracers-substeps", "2", "--tracers-mobility", "1e-9"]
    plain = _run_driver([*geo, *flags], tmp_path / "plain")
    loop = _run_driver([*geo, *flags, "--tracers-sort-every", "3"], tmp_path / "loop")
    batch = _run_driver([*geo, *flags, "--tracers-sort-every", "3", "--batch", "1"], tmp_path / "batch")
    assert sorted(os.listdir(loop)) == sorted(os.listdir(plain)) == sorted(os.listdir(batch))
    for f in os.listdir(loop):
        assert (loop / f).read_bytes() == (batch / f).read_bytes(), f
        if not f.startswith("tracers"):
            assert (loop / f).read_bytes() == (plain / f).read_bytes(), f
    want, none, r0 = _parse((plain / "tracers_final.bin").read_bytes())
    got, ids, r1 = _parse((loop / "tracers_final.bin").read_bytes())
    assert (r0, r1) == (0, 1) and none is None and np.array_equal(np.sort(ids), np.arange(n)) and not np.array_equal(ids, np.arange(n))
    for name in ARRAYS:
        back = np.empty_like(got[name])
        back[ids] = got[name]
        assert _same_array(back, want[name]), name
    rows = [np.array([[float(v) for v in ln.split(" ")] for ln in (d / "tracers.dat").read_text().splitlines()[2:]]) for d in (plain, loop)]
    assert rows[0].shape == (6, 14) and rows[1].shape == (6, 14)
    exact = [0, 1, 2, 3, 12, 13]   # step, time, alive, lost, z_min, z_max
    assert np.array_equal(rows[0][:, exact], rows[1][:, exact])
    # the sums are added in slot order: each run's last row against the exact sum of the final cloud's terms
    alive = ~np.isnan(want["x"])
    dx = (want["x"][alive] - want["x0"][alive]) + want["wx"][alive].astype(np.float64) * 40.0
    dy = (want["y"][alive] - want["y0"][alive]) + want["wy"][alive].astype(np.float64) * 12.0
    dz = want["z"][alive] - want["z0"][alive]
    za = want["z"][alive]
    for k, t in enumerate([dx, dy, dz, dx * dx, dy * dy, dz * dz, za, za * za]):
        tol = n * 2.0 ** -53 * np.abs(t).sum()
        for r, which in zip(rows, ("plain", "sorted")):
            d = abs(r[-1, 4 + k] - math.fsum(t))
            print(f"{pkg.TRACER_MOMENTS[2 + k]} {which}: {d:.3e} (tol {tol:.3e})")
            assert d <= tol, (pkg.TRACER_MOMENTS[2 + k], which, d, tol)
