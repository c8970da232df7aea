"""GPU tests of the Brownian tracers (csrc/tracers.hip: k_tracers_advance_brownian; include/ekpnp.h: ekpnp_tracers_advance_brownian,
ekpnp_tracers_epoch; `ekpnp_main --tracers-diffusivity D`).

ekpnp_tracers_advance_brownian_host is the definition (tests/test_tracers_brownian_cpu.py holds it against a numpy transcription), so the
device is compared with it EXACTLY: all eight arrays of the cloud, read through the cloud's own file, on their bit pattern.  Nothing
here has a tolerance.

Lattices: W 70 x 66 x 13, O 35 x 33 x 5 (odd: the planes start at odd doubles), R 40 x 12 x 17 and T 70 x 66 x 17 of the tracer tests.
n = 1 (one lane), 63 / 64 / 65 (a wavefront and either side), 257 (one past a workgroup), 1000 (a ragged workgroup), 4097."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _tracers_brownian_ref as B
import _tracers_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
SHAPES = {"W": (70, 66, 13), "O": (35, 33, 5), "R": (40, 12, 17), "T": (70, 66, 17)}
NS = (1, 63, 64, 65, 257, 1000, 4097)
UE = ("ux", "uy", "uz", "Ex", "Ey", "Ez")
ARRAYS = ("x", "y", "z", "x0", "y0", "z0", "wx", "wy")
NOISE = 0xC0FFEE1234567


def _params(pkg, shape, in_place=0):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    p.in_place = in_place
    return p


@pytest.fixture(scope="module")
def inputs(pkg):
    """per lattice: (u, E) random fields and a cloud of 4097 positions - the special ones in front, some next to the plates; made
    once, never modified"""
    out = {}
    for k, s in SHAPES.items():
        u, E = T.random_fields(s, 281 + len(out), T.U_SCALE, T.E_SCALE)
        x, y, z = B.plate_cloud(s, 4097, 291 + len(out))
        for a in (*u, *E, x, y, z):
            a.setflags(write=False)
        out[k] = (u, E, x, y, z)
    return out


@pytest.fixture(scope="module")
def host(pkg, inputs):
    """host(shape, n, nsub, mu, epoch=0) -> ekpnp_tracers_advance_brownian_host of the first n particles; computed once per case, never
    modified"""
    cache = {}

    def get(shape, n, nsub, mu, epoch=0):
        key = (shape, n, nsub, mu, epoch)
        if key not in cache:
            u, E, x, y, z = inputs[shape]
            p = pkg.default_params(*SHAPES[shape])
            cache[key] = pkg.tracers_advance_brownian_host(p, u, x[:n], y[:n], z[:n], E=E, mu=mu, D=B.diffusivity(p), h=T.substep(p), nsub=nsub,
                                                           seed=NOISE, epoch=epoch)
            for a in cache[key]:
                a.setflags(write=False)
        return cache[key]

    return get


def _put_fields(s, u, E):
    for name, a in zip(UE, (*u, *E)):
        s.set_field(name, a)


def _parse(raw):
    """the cloud's file: ({x, y, z, x0, y0, z0, wx, wy}, ids or None, reserved, reserved2)"""
    assert raw[:8] == b"EKPNPTR1"
    reserved = int(np.frombuffer(raw[20:24], dtype="<i4")[0])
    n = int(np.frombuffer(raw[24:32], dtype="<i8")[0])
    assert len(raw) == 48 + (60 if reserved == 1 else 56) * n, (len(raw), reserved, n)
    d = np.frombuffer(raw[48:48 + 48 * n], dtype="<f8").reshape(6, n)
    w = np.frombuffer(raw[48 + 48 * n:48 + 56 * n], dtype="<i4").reshape(2, n)
    ids = np.frombuffer(raw[48 + 56 * n:], dtype="<i4") if reserved == 1 else None
    return dict(zip(ARRAYS, [*d, *w])), ids, reserved, int(np.frombuffer(raw[40:48], dtype="<i8")[0])


def _dump(s, path):
    s.tracers_save(str(path), time=0.5)
    return _parse(open(path, "rb").read())


def _assert_eight(cloud, start, want, what):
    """all eight arrays: the position and the image counts are the host's, the start is the start"""
    for k, name in enumerate(("x", "y", "z")):
        assert T.same(cloud[name], want[k]), (what, name, np.flatnonzero(T.bits(cloud[name]) != T.bits(want[k]))[:5])
        assert T.same(cloud[name + "0"], start[k]), (what, name + "0")
    assert cloud["wx"].dtype == np.int32 and np.array_equal(cloud["wx"], want[3]) and np.array_equal(cloud["wy"], want[4]), what


def _assert_cloud(got, want, what):
    for k, name in enumerate(("x", "y", "z")):
        assert T.same(got[k], want[k]), (what, name, np.flatnonzero(T.bits(got[k]) != T.bits(want[k]))[:5])
    assert got[3].dtype == np.int32 and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]), what


def _brownian(s, nsub, mu, **kw):
    s.tracers_advance(T.substep(s.p), nsub=nsub, mu=mu, D=B.diffusivity(s.p), seed=NOISE, **kw)


# ---- 1. the device equals the definition -----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["W", "O", "R", "T"])
def test_device_brownian_advance_equals_the_host_definition(pkg, inputs, host, shape, tmp_path):
    """fails on the parent commit: ekpnp_tracers_advance_brownian and its host definition do not exist there"""
    u, E, x, y, z = inputs[shape]
    p = _params(pkg, SHAPES[shape])
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        for n in NS:
            for nsub in (1, 7):
                for mu in (0.0, T.MU):
                    s.tracers_set(x[:n], y[:n], z[:n])
                    assert s.tracers_size == n and s.tracers_epoch() == 0
                    _brownian(s, nsub, mu)
                    cloud, ids, reserved, reserved2 = _dump(s, tmp_path / "c.bin")
                    want = host(shape, n, nsub, mu)
                    _assert_eight(cloud, (x[:n], y[:n], z[:n]), want, (shape, n, nsub, mu))
                    assert ids is None and reserved == 0 and reserved2 == nsub and s.tracers_epoch() == nsub
                    if n >= 1000:
                        assert np.isnan(cloud["x"][12]) and np.isnan(cloud["x"]).sum() == np.isnan(want[0]).sum()
        # the cases did happen: wraps either way, reflections at both plates (nobody is held by one), and the noise moved everybody
        got = s.tracers_get()
        plain = pkg.tracers_advance_host(p, u, x, y, z, E=E, mu=T.MU, h=T.substep(p), nsub=7)
        alive = ~np.isnan(got[0]) & ~np.isnan(plain[0])
        assert (got[3] > 0).any() and (got[3] < 0).any() and (got[4] > 0).any() and (got[4] < 0).any()
        assert (got[0][alive] != plain[0][alive]).all()
        top = float(SHAPES[shape][2] - 1)
        ok = ~np.isnan(z)
        raw = z[ok] + B.kick_lengths(p, B.diffusivity(p), T.substep(p))[2] * B.kick(NOISE, np.flatnonzero(ok), 0)[2]   # the first kick, had there been no flow
        assert (raw < 0.0).sum() >= 10 and (raw > top).sum() >= 10
        assert (got[2][alive] > 0.0).all() and (got[2][alive] < top).all()


def test_in_place_and_a_bound_array_give_the_same_bits(pkg, inputs, host):
    import torch

    u, E, x, y, z = inputs["W"]
    with pkg.Solver(_params(pkg, SHAPES["W"], in_place=1)) as s:
        _put_fields(s, u, E)
        for mu in (0.0, T.MU):
            s.tracers_set(x[:1000], y[:1000], z[:1000])
            _brownian(s, 7, mu)
            _assert_cloud(s.tracers_get(), host("W", 1000, 7, mu), ("in place", mu))
    with pkg.Solver(_params(pkg, SHAPES["W"])) as s:  # ux at an address that is 8 mod 16
        n = int(np.prod(s.shape))
        pool = torch.zeros(n + 3, dtype=torch.float64, device="cuda")
        view = pool[1:1 + n] if pool.data_ptr() % 16 == 0 else pool[2:2 + n]
        assert view.data_ptr() % 16 == 8
        s.bind_field("ux", view.data_ptr())
        _put_fields(s, u, E)
        for mu in (0.0, T.MU):
            s.tracers_set(x[:1000], y[:1000], z[:1000])
            _brownian(s, 7, mu)
            _assert_cloud(s.tracers_get(), host("W", 1000, 7, mu), ("bound", mu))
        s.synchronize()
        off = (view.data_ptr() - pool.data_ptr()) // 8
        assert float(pool[:off].abs().sum()) == 0.0 and float(pool[off + n:].abs().sum()) == 0.0  # the guard elements are untouched


SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)


def _seeded_start(pkg, s, **knobs):
    for k, v in knobs.items():
        s.tune(k, v)
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


def test_after_real_steps_the_advance_reads_the_fields_get_field_returns(pkg):
    """lazy E is on: after step(3) the E arrays are older than phi.  A charged Brownian advance must bring them up to date first (it
    then equals the host definition on what a twin's get_field returns); a passive one reads u only, and the run goes on as the
    twin's."""
    p = _params(pkg, SHAPES["R"])
    spec = pkg.tracers_spec(n=1000, p=p, seed=3)
    x0, y0, z0 = pkg.tracers_seed_host(p, spec)
    with pkg.Solver(p) as a, pkg.Solver(p) as b, pkg.Solver(p) as c:
        for s in (a, b, c):
            _seeded_start(pkg, s)
            s.step(3)
        f = c.fields()
        u, E = [f[k] for k in UE[:3]], [f[k] for k in UE[3:]]
        umax, emax = max(np.abs(v).max() for v in u), max(np.abs(v).max() for v in E)
        assert umax > 0.0 and emax > 0.0
        h = 0.5 * p.dx / umax                 # the fastest node moves a particle half a cell per substep, mu E as far, a kick up to a cell
        mu = 0.5 * umax / emax
        D = p.dx ** 2 / (6.0 * h)
        a.tracers_seed(spec)
        a.tracers_advance(h, nsub=5, mu=mu, D=D, seed=9)
        want = pkg.tracers_advance_brownian_host(p, u, x0, y0, z0, E=E, mu=mu, D=D, h=h, nsub=5, seed=9)
        _assert_cloud(a.tracers_get(), want, "charged")
        passive = pkg.tracers_advance_brownian_host(p, u, x0, y0, z0, mu=0.0, D=D, h=h, nsub=5, seed=9)
        assert not T.same(passive[0], want[0]) and np.isnan(want[0]).sum() < 100
        b.tracers_seed(spec)
        b.tracers_advance(h, nsub=5, mu=0.0, D=D, seed=9)   # lazy E is left alone: nothing but u is read
        for s in (a, b, c):
            s.step(3)
        _assert_cloud(b.tracers_get(), passive, "passive")
        fa, fb, fc = a.fields(), b.fields(), c.fields()
        for n in pkg.FIELDS:
            assert np.array_equal(T.bits(fa[n]), T.bits(fc[n])) and np.array_equal(T.bits(fb[n]), T.bits(fc[n])), n


# ---- 2. the epoch ------------------------------------------------------------------------------------------------------

def test_successive_calls_equal_one_host_run_over_the_joined_epochs(pkg, inputs, host):
    u, E, x, y, z = inputs["W"]
    p = _params(pkg, SHAPES["W"])
    with pkg.Solver(p) as s:
        _put_fields(s, u, E)
        assert s.tracers_epoch() == 0   # no cloud
        s.tracers_set(x[:1000], y[:1000], z[:1000])
        _brownian(s, 3, T.MU)
        assert s.tracers_epoch() == 3
        _brownian(s, 4, T.MU)
        assert s.tracers_epoch() == 7
        whole = host("W", 1000, 7, T.MU)
        _assert_cloud(s.tracers_get(), whole, "3 + 4")
        # a plain advance takes no epoch, a third Brownian call goes on from 7
        s.tracers_advance(T.substep(p), nsub=2, mu=T.MU)
        assert s.tracers_epoch() == 7
        mid = pkg.tracers_advance_host(p, u, *whole, E=E, mu=T.MU, h=T.substep(p), nsub=2)
        _brownian(s, 2, 0.0)
        assert s.tracers_epoch() == 9
        want = pkg.tracers_advance_brownian_host(p, u, *mid, mu=0.0, D=B.diffusivity(p), h=T.substep(p), nsub=2, seed=NOISE, epoch=7)
        _assert_cloud(s.tracers_get(), want, "from epoch 7")
        again = pkg.tracers_advance_brownian_host(p, u, *mid, mu=0.0, D=B.diffusivity(p), h=T.substep(p), nsub=2, seed=NOISE, epoch=0)
        assert not T.same(again[0], want[0])
        # seed and set start the clock again
        s.tracers_set(x[:1000], y[:1000], z[:1000])
        assert s.tracers_epoch() == 0
        _brownian(s, 7, T.MU)
        _assert_cloud(s.tracers_get(), whole, "after set")
        s.tracers_seed(n=100, seed=1)
        assert s.tracers_epoch() == 0
        s.tracers_release()
        assert s.tracers_epoch() == 0


def test_a_sorted_cloud_draws_the_numbers_of_its_unsorted_twin(pkg, inputs, host):
    """the noise is keyed by the particle's id, not by its slot: this fails if k_tracers_advance_brownian uses the slot"""
    u, E, x, y, z = inputs["T"]
    p = _params(pkg, SHAPES["T"])
    n = 4097
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        for s in (a, b):
            _put_fields(s, u, E)
            s.tracers_set(x[:n], y[:n], z[:n])
        a.tracers_sort()
        ids = a.tracers_ids()
        assert (ids != np.arange(n)).sum() > n // 2   # the sort did move the particles
        for s in (a, b):
            _brownian(s, 3, T.MU)
        _assert_cloud(a.tracers_get(by_id=True), b.tracers_get(), "sorted, then advanced")
        a.tracers_sort()                              # a stirred cloud, sorted again: the ids are composed
        assert not np.array_equal(a.tracers_ids(), ids)
        for s in (a, b):
            _brownian(s, 4, T.MU)
        _assert_cloud(a.tracers_get(by_id=True), b.tracers_get(), "sorted twice")
        _assert_cloud(b.tracers_get(), host("T", n, 7, T.MU), "the twin")
        assert a.tracers_epoch() == 7 and b.tracers_epoch() == 7


# ---- 3. the cloud's file -----------------------------------------------------------------------------------------------

def test_save_load_and_continue_is_not_having_stopped(pkg, inputs, host, tmp_path):
    u, E, x, y, z = inputs["W"]
    p = _params(pkg, SHAPES["W"])
    path = str(tmp_path / "cloud.bin")
    n = 1000
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        _put_fields(a, u, E)
        _put_fields(b, u, E)
        # a cloud that never took a Brownian substep writes the bytes it always wrote
        a.tracers_set(x[:n], y[:n], z[:n])
        a.tracers_advance(T.substep(p), nsub=2, mu=T.MU)
        a.tracers_save(path, time=0.25)
        g = a.tracers_get()
        hdr = b"EKPNPTR1" + np.array([70, 66, 13, 0], "<i4").tobytes() + np.array([n], "<i8").tobytes() + np.array([0.25], "<f8").tobytes() + np.array([0], "<i8").tobytes()
        body = b"".join(np.ascontiguousarray(v, "<f8").tobytes() for v in (g[0], g[1], g[2], x[:n], y[:n], z[:n])) + g[3].tobytes() + g[4].tobytes()
        assert open(path, "rb").read() == hdr + body
        # three Brownian substeps, saved, loaded by a twin, four more on both: the host's seven
        a.tracers_set(x[:n], y[:n], z[:n])
        _brownian(a, 3, T.MU)
        a.tracers_save(path, time=0.125)
        raw = open(path, "rb").read()
        cloud, ids, reserved, reserved2 = _parse(raw)
        assert len(raw) == 48 + 56 * n and ids is None and reserved == 0 and reserved2 == 3 == a.tracers_epoch()
        assert b.tracers_epoch() == 0
        assert b.tracers_load(path) == 0.125 and b.tracers_size == n and b.tracers_epoch() == 3
        for s in (a, b):
            _brownian(s, 4, T.MU)
        _assert_cloud(b.tracers_get(), a.tracers_get(), "continued")
        _assert_cloud(b.tracers_get(), host("W", n, 7, T.MU), "as if it had not stopped")
        assert T.same(b.tracers_moments(), a.tracers_moments())
        # a sorted, diffused cloud: ids and epoch both travel
        a.tracers_sort()
        a.tracers_save(path, time=0.5)
        _, ids, reserved, reserved2 = _parse(open(path, "rb").read())
        assert reserved == 1 and reserved2 == 7 and np.array_equal(ids, a.tracers_ids())
        b.tracers_load(path)
        assert b.tracers_epoch() == 7 and np.array_equal(b.tracers_ids(), ids)
        for s in (a, b):
            _brownian(s, 2, 0.0)
        _assert_cloud(b.tracers_get(), a.tracers_get(), "sorted and continued")
        _assert_cloud(a.tracers_get(by_id=True), pkg.tracers_advance_brownian_host(p, u, *host("W", n, 7, T.MU), D=B.diffusivity(p), h=T.substep(p), nsub=2,
                                                                                   seed=NOISE, epoch=7), "sorted, by id")
        # a negative epoch in a file is refused, with the number, and the cloud is left alone
        before = b.tracers_get()
        bad = bytearray(raw)
        bad[40:48] = np.array([-5], "<i8").tobytes()
        open(tmp_path / "negative.bin", "wb").write(bytes(bad))
        with pytest.raises(pkg.EkpnpError) as e:
            b.tracers_load(str(tmp_path / "negative.bin"))
        assert "reserved2 = -5" in str(e.value) and "status 1" in str(e.value)
        _assert_cloud(b.tracers_get(), before, "a refused load")
        assert b.tracers_epoch() == 9


# ---- 4. no diffusivity, and the run is left alone ----------------------------------------------------------------------

def test_no_diffusivity_equals_the_plain_device_advance(pkg, inputs):
    u, E, x, y, z = inputs["O"]
    p = _params(pkg, SHAPES["O"])
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        for s in (a, b):
            _put_fields(s, u, E)
        for mu in (0.0, T.MU):
            for h in (T.substep(p), -T.substep(p)):
                for s in (a, b):
                    s.tracers_set(x, y, z)
                a.tracers_advance(h, nsub=7, mu=mu, D=0.0, seed=NOISE)
                b.tracers_advance(h, nsub=7, mu=mu)
                ga, gb = a.tracers_get(), b.tracers_get()
                for k in range(5):
                    assert np.array_equal(ga[k], gb[k], equal_nan=True), (mu, h, k)
                assert a.tracers_epoch() == 7 and b.tracers_epoch() == 0


def test_brownian_advances_leave_the_step_graph_and_the_run_alone(pkg):
    p = _params(pkg, SHAPES["R"])
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        _seeded_start(pkg, a)
        _seeded_start(pkg, b)
        a.step(5)
        b.step(5)
        state = a.graph_state()
        assert state == 1
        before = a.device_bytes()
        a.tracers_seed(n=1000, seed=1)
        with_cloud = a.device_bytes()
        D = (0.5 * p.dx) ** 2 / (6.0 * p.dt)
        for k in range(6):
            a.step(1)
            a.tracers_advance(p.dt, nsub=2, mu=1e-8 if k % 2 else 0.0, D=D, seed=k)
            assert a.device_bytes() == with_cloud   # the kernel needs nothing but the cloud
        b.step(6)
        assert a.graph_state() == state and b.graph_state() == state and a.tracers_epoch() == 12
        fa, fb = a.fields(), b.fields()
        for n in pkg.FIELDS:
            assert np.array_equal(T.bits(fa[n]), T.bits(fb[n])), n
        assert b.device_bytes() == before
        a.tracers_release()
        assert a.device_bytes() == before


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as G
pkg = G.load_package()
p = pkg.default_params(40, 12, 17)
with pkg.Solver(p) as s:
    s.tracers_seed(n=5000, seed=1)
    s.tracers_advance(1e-9, nsub=2)
    s.tracers_advance(1e-9, nsub=2, mu=1e-8)
    s.tracers_sort(); s.tracers_moments(); s.tracers_cell_counts((4, 3, 2)); s.tracers_sample(["ux"]); s.tracers_save(sys.argv[1])
    print("PLAIN OK", s.tracers_epoch())
    try:
        s.tracers_advance(1e-9, nsub=2, D=1e-9)
        print("BROWNIAN OK")
    except pkg.EkpnpError as e:
        print("ERR", e)
''' % ROOT


def test_a_context_that_never_diffuses_launches_no_brownian_kernel(tmp_path):
    """the library's launch-failure knob (read once per process, hence a child) fails the named kernel's first launch: everything a
    cloud did before this change goes through, and the Brownian advance reports that kernel by name"""
    env = dict(os.environ, EKPNP_INJECT_LAUNCH_FAILURE="k_tracers_advance_brownian")
    r = subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "c.bin")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "PLAIN OK 0" in r.stdout and "ERR" in r.stdout and "kernel k_tracers_advance_brownian:" in r.stdout, (r.stdout, r.stderr[-2000:])
    assert os.path.getsize(tmp_path / "c.bin") == 48 + 60 * 5000


# ---- 5. refusals -------------------------------------------------------------------------------------------------------

def test_refusals_of_the_context_calls(pkg):
    p = _params(pkg, SHAPES["W"])
    msg = "tracers: slab contexts are not supported"
    for rank, nranks in ((0, 1), (1, 3)):
        with pkg.Solver(p, rank=rank, nranks=nranks, slab=True) as s:
            for k, call in enumerate((lambda: s.tracers_advance(1e-9, D=1e-9), lambda: s.tracers_epoch())):
                with pytest.raises(pkg.EkpnpError) as e:
                    call()
                assert "status 1" in str(e.value) and msg in str(e.value), k
    assert not [m for m in dir(pkg.Group) if "tracers" in m]   # and a group has no spelling of them
    with pkg.Solver(p) as s:
        with pytest.raises(pkg.EkpnpError) as e:
            s.tracers_advance(1e-9, D=1e-9)
        assert "no cloud" in str(e.value)
        s.tracers_seed(n=100, seed=1)
        before = s.tracers_get()
        for kw, number in ((dict(h=1e-9, D=-1.5), "D = -1.5"), (dict(h=1e-9, D=float("nan")), "D = nan"), (dict(h=-0.25, D=0.5), "D*h = -0.125"),
                           (dict(h=1e-9, D=1e-9, nsub=0), "nsub = 0"), (dict(h=1e-9, D=1e-9, nsub=4097), "nsub = 4097"),
                           (dict(h=float("inf"), D=1e-9), "h = inf"), (dict(h=1e-9, D=1e-9, mu=float("inf")), "mu = inf")):
            with pytest.raises(pkg.EkpnpError) as e:
                s.tracers_advance(**kw)
            assert number in str(e.value) and "status 1" in str(e.value), kw
        assert s.tracers_epoch() == 0   # a refused call takes no epoch and moves nobody
        _assert_cloud(s.tracers_get(), before, "refused")


# ---- 6. the driver -----------------------------------------------------------------------------------------------------

def _run_driver(args, out, code=0):
    out.mkdir()
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1", EKPNP_PLACEMENT_TRIES="1")  # the child shares device 0 with this process
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == code, (args, r.stderr[-2000:])
    return out, r.stderr


GEO = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "6", "--seed-pattern", "squares", "--seed-modes", "1,1"]


def test_driver_writes_the_files_of_the_library_calls_in_both_loops(pkg, tmp_path):
    assert os.path.exists(EXE), "ekpnp_main not built"
    p = pkg.default_params(40, 12, 17)
    mu = 1e-9
    D = (0.5 * p.dx) ** 2 / (12.0 * p.dt)   # a kick of up to half a cell per substep of 2 dt
    spec = pkg.tracers_spec(n=1000, box=((0, 40), (0, 12), (1, 15)), seed=9)
    with pkg.Solver(p) as s:  # the driver's loop, call by call
        s.initialization()
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-3, noise=0.0, relative=True, seed=1))
        s.fast_Poisson()
        s.init_equilibrium()
        s.tracers_seed(spec)
        s.tracers_arm(3)
        t = 0.0
        for i in range(6):
            s.stream_collide_save(t)
            s.fast_Poisson()
            t = t + p.dt
            if (i + 1) % 2 == 0:
                s.tracers_advance(2.0 * p.dt, nsub=3, mu=mu, D=D, seed=77)
                s.tracers_record(i + 1, t)
        s.tracers_ring_save(str(tmp_path / "lib_tracers.dat"))
        s.tracers_save(str(tmp_path / "lib_final.bin"), time=t)
        counts, lost = s.tracers_cell_counts((4, 3, 2))
        moved = s.tracers_moments()
    assert moved[5] / moved[0] > 0.05   # mean dx^2 of nine kicks of up to half a cell: the noise is in the files
    flags = ["--tracers", "1000", "--tracers-seed", "9", "--tracers-every", "2", "--tracers-substeps", "3", "--tracers-mobility", "1e-9", "--tracers-cells", "4,3,2"]
    noise = ["--tracers-diffusivity", repr(D), "--tracers-noise-seed", "77"]
    quiet, _ = _run_driver([*GEO, *flags], tmp_path / "quiet")
    loop, _ = _run_driver([*GEO, *flags, *noise], tmp_path / "loop")
    batch, _ = _run_driver([*GEO, *flags, *noise, "--batch", "1"], tmp_path / "batch")
    assert (loop / "tracers.dat").read_bytes() == (tmp_path / "lib_tracers.dat").read_bytes()
    assert (loop / "tracers_final.bin").read_bytes() == (tmp_path / "lib_final.bin").read_bytes()
    assert _parse((loop / "tracers_final.bin").read_bytes())[3] == 9 and _parse((quiet / "tracers_final.bin").read_bytes())[3] == 0
    cells = (loop / "tracer_cells.dat").read_text().splitlines()
    assert cells[0].startswith("# ekpnp tracer cells nx 40 ny 12 nz 17 bx 4 by 3 bz 2 n 1000 lost %d time " % lost)
    assert np.array_equal(np.array([[int(v) for v in ln.split(" ")] for ln in cells[1:]]).reshape(2, 3, 4), counts)
    for f in ("tracers.dat", "tracers_final.bin", "tracer_cells.dat"):
        assert (loop / f).read_bytes() == (batch / f).read_bytes(), f
    assert (loop / "tracers_final.bin").read_bytes() != (quiet / "tracers_final.bin").read_bytes()
    for f in ("data.dat", "umax.dat", "data_end.dat"):
        v = (quiet / f).read_bytes()
        assert len(v) > 0 and v == (loop / f).read_bytes() and v == (batch / f).read_bytes(), f
    assert sorted(os.listdir(loop)) == sorted(os.listdir(quiet))
    for bad, number in ((["--tracers-diffusivity", "1e-9"], "there is no cloud to diffuse"), (["--tracers-noise-seed", "3"], "there is no cloud to diffuse"),
                        (["--tracers", "10", "--tracers-noise-seed", "3"], "--tracers-noise-seed 3"), (["--tracers", "10", "--tracers-diffusivity", "fast"], "got fast"),
                        (["--tracers", "10", "--tracers-diffusivity", "-2.5"], "D = -2.5"), (["--tracers", "10", "--tracers-diffusivity", "1e-9", "--tracers-noise-seed", "x"], "got x")):
        _, err = _run_driver([*GEO, *bad], tmp_path / ("bad" + "_".join(bad).replace("-", "").replace(",", "_")), code=2)
        assert number in err, err
