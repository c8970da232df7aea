"""GPU tests of sampling the fields at the tracers and of the tracks of tagged particles (csrc/tracers.hip: k_tracers_sample,
k_tracers_track_find, k_tracers_track_row; include/ekpnp.h: ekpnp_tracers_sample*, ekpnp_tracks_*; `ekpnp_main --tracks-first K`).

ekpnp_tracers_sample_host is the definition (tests/test_tracers_sample_cpu.py holds it against a numpy transcription), so the device is
compared with it on the float64 BIT PATTERN; a lost particle's NaN is compared by isnan; counts and ids are integers.  No tolerance
appears anywhere.  Lattices W 70 x 66 x 13, O 35 x 33 x 5, R 40 x 12 x 17 and clouds of n = 1 (one lane), 1000 (not a multiple of 256) and 4097
(one past a run of 4096, and not a multiple of the find's four ids per thread), as in the other tracer tests."""
import os
import subprocess

import numpy as np
import pytest

import _tracers_ref as T
import _tracers_sample_ref as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
SLAB_MSG = "tracers: slab contexts are not supported"


def _params(pkg, shape, in_place=0):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    p.in_place = in_place
    return p


@pytest.fixture(scope="module")
def fields():
    """per lattice: the eleven random fields; made once, never modified"""
    return {k: S.all_fields(s, 950 + i) for i, (k, s) in enumerate(S.SHAPES.items())}


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(T.bits(a), T.bits(b))


# ---- 1. the device equals the definition -----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_device_sample_equals_sample_host(pkg, fields, shape):
    import torch

    dims = S.SHAPES[shape]
    p = _params(pkg, dims)
    f = fields[shape]
    with pkg.Solver(p) as s:
        s.set_fields(f)
        for n in S.NS:
            x, y, z = T.special_cloud(dims, n, 60 + n)
            s.tracers_set(x, y, z)
            for name, values in S.VALUE_SETS.items():
                want = pkg.tracers_sample_host(p, values, f, x, y, z)
                got = s.tracers_sample(values)
                assert S.same_sample(got, want), (shape, n, name)
                out = torch.full((len(values), n), -7.0, dtype=torch.float64, device="cuda")
                s.tracers_sample_into(values, out)
                s.synchronize()
                assert S.same_sample(out.cpu().numpy(), want), (shape, n, name, "into a tensor")
            if n >= 1000:
                assert np.isnan(want[:, 12]).all() and np.isnan(want).sum() == 12   # exactly the lost particle


def test_in_place_and_a_bound_array(pkg, fields):
    import torch

    dims = S.SHAPES["W"]
    f = fields["W"]
    n = 4097
    x, y, z = T.special_cloud(dims, n, 70)
    want = pkg.tracers_sample_host(_params(pkg, dims), S.NAMES, f, x, y, z)
    with pkg.Solver(_params(pkg, dims, in_place=1)) as s:
        s.set_fields(f)
        s.tracers_set(x, y, z)
        assert S.same_sample(s.tracers_sample(S.NAMES), want)
    with pkg.Solver(_params(pkg, dims)) as s:   # T at an address that is 8 mod 16
        m = int(np.prod(s.shape))
        pool = torch.zeros(m + 3, dtype=torch.float64, device="cuda")
        view = pool[1:1 + m] if pool.data_ptr() % 16 == 0 else pool[2:2 + m]
        s.bind_field("T", view.data_ptr())
        s.set_fields(f)
        s.tracers_set(x, y, z)
        assert S.same_sample(s.tracers_sample(S.NAMES), want)
        assert S.same_sample(s.tracers_sample(["T"]), want[10:11])


# ---- 2. after real steps: the arrays get_field returns, and lazy E ---------------------------------------------------------

SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)


def _seeded_start(pkg, s, **knobs):
    for k, v in knobs.items():
        s.tune(k, v)
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


@pytest.mark.parametrize("lazy", [1, 0])
def test_after_steps_the_sample_reads_what_get_field_returns(pkg, lazy):
    dims = S.SHAPES["R"]
    p = _params(pkg, dims)
    n = 1000
    x, y, z = T.special_cloud(dims, n, 80)
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        for s in (a, b):
            _seeded_start(pkg, s, lazy_efield=lazy)
            s.tracers_set(x, y, z)
            s.step(5)
        state = a.graph_state()
        # T alone: lazy E is left alone - the twin b, which never sampled, goes on to the same bits
        got = a.tracers_sample(["T", "q", "uz"])
        assert a.graph_state() == state
        a.step(2)
        b.step(2)
        fa, fb = a.fields(), b.fields()
        for name in pkg.FIELDS:
            assert _bits_equal(fa[name], fb[name]), name
        want = pkg.tracers_sample_host(p, ["T", "q", "uz"], fb, x, y, z)
        assert S.same_sample(a.tracers_sample(["T", "q", "uz"]), want)
        a.step(3)
        b.step(3)
        # Ez and phi named FIRST after the steps: the bits of the up-to-date arrays
        got = a.tracers_sample(["Ez", "phi", "Ex", "c"])
        fb = b.fields()
        assert S.same_sample(got, pkg.tracers_sample_host(p, ["Ez", "phi", "Ex", "c"], fb, x, y, z))
        assert S.same_sample(a.tracers_sample(S.NAMES), pkg.tracers_sample_host(p, S.NAMES, fb, x, y, z))
        assert a.graph_state() == state
        a.step(2)
        b.step(2)
        fa, fb = a.fields(), b.fields()
        for name in pkg.FIELDS:
            assert _bits_equal(fa[name], fb[name]), name


# ---- 3. after a sort ---------------------------------------------------------------------------------------------------

def test_a_sort_permutes_the_sample_and_by_id_undoes_it(pkg, fields):
    dims = S.SHAPES["W"]
    p = _params(pkg, dims)
    f = fields["W"]
    values = ["T", "q", "ux", "Ez"]
    with pkg.Solver(p) as s:
        s.set_fields(f)
        for n in S.NS:
            x, y, z = T.special_cloud(dims, n, 90 + n)
            s.tracers_set(x, y, z)
            before = s.tracers_sample(values)
            assert S.same_sample(before, s.tracers_sample(values, by_id=True))   # never sorted: slot == id
            s.tracers_sort()
            ids = s.tracers_ids()
            assert n < 1000 or not np.array_equal(ids, np.arange(n))
            assert S.same_sample(s.tracers_sample(values, by_id=True), before), n
            assert S.same_sample(s.tracers_sample(values), before[:, ids]), n


# ---- 4. tracks ---------------------------------------------------------------------------------------------------------

def _twin_row(s, ids, values):
    """what a row must hold, from the synchronous calls: [ntags, 5 + nvalues]"""
    x, y, z, wx, wy = s.tracers_get(by_id=True)
    cols = [x[ids], y[ids], z[ids], wx[ids].astype(np.float64), wy[ids].astype(np.float64)]
    if len(values):
        v = s.tracers_sample(values, by_id=True)
        cols += [v[k][ids] for k in range(len(values))]
    return np.stack(cols, axis=1)


def _same_rows(got, want):
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(T.bits(got)[~nan], T.bits(want)[~nan])


@pytest.mark.parametrize("batch, stride", [(0, 1), (1, 3)])
@pytest.mark.parametrize("ntags, values", [(1, ()), (5, ("T", "q", "uz")), (300, ("T", "q", "uz")), (300, ())])
def test_track_rows_equal_a_twin(pkg, ntags, values, batch, stride, tmp_path):
    dims = S.SHAPES["R"]
    p = _params(pkg, dims)
    n = 4097
    x, y, z = T.special_cloud(dims, n, 100)
    ids = np.random.default_rng(ntags).permutation(n)
    ids = ids[ids != 12][:ntags].astype(np.int64)   # scrambled order
    if ntags >= 5:
        ids[1] = 12   # the particle that is lost from the start
    h = 40 * p.dt
    rows, labels = [], []
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        for s in (a, b):
            _seeded_start(pkg, s, batch_moments=batch)
            s.tracers_set(x, y, z)
            s.step(4)
        a.tracks_arm(ids=ids, values=values, capacity=3)
        assert a.tracks_count() == (0, 0)
        for k in range(5):
            for s in (a, b):
                s.step(stride)
                if k == 2 or k == 4:
                    s.tracers_sort()   # in the middle, and a second one
                s.tracers_advance(h, nsub=2, mu=1e-8 if k % 2 else 0.0)
            a.tracks_record(10 + k, 0.25 * k)
            rows.append(_twin_row(b, ids, values))
            labels.append((10 + k, 0.25 * k))
        assert not np.array_equal(b.tracers_ids(), np.arange(n))
        assert a.tracks_count() == (5, 2)
        steps, times, got = a.tracks_read()
        assert got.shape == (3, ntags, 5 + len(values))
        assert steps.tolist() == [12, 13, 14] and times.tolist() == [0.5, 0.75, 1.0]
        for r in range(3):
            assert _same_rows(got[r], rows[2 + r]), (ntags, values, r)
        if ntags >= 5:
            assert np.isnan(got[:, 1, :3]).all() and np.isnan(got[:, 1, 5:]).all() and not np.isnan(got[:, 1, 3:5]).any()
        s1, t1, one = a.tracks_read(1, 1)
        assert s1.tolist() == [13] and _same_rows(one[0], rows[3])
        with pytest.raises(pkg.EkpnpError) as e:
            a.tracks_read(1, 3)
        assert "3 held" in str(e.value)
        # the file: %.17g round-trips
        path = tmp_path / "tracks.dat"
        a.tracks_save(str(path))
        lines = path.read_text().splitlines()
        assert lines[0] == f"# ekpnp tracks nx 40 ny 12 nz 17 n {n} ntags {ntags} nvalues {len(values)} recorded 5 dropped 2"
        assert lines[1] == " ".join(["# step time id x y z wx wy", *values])
        assert len(lines) == 2 + 3 * ntags
        for r in range(3):
            for t in range(ntags):
                w = lines[2 + r * ntags + t].split(" ")
                assert (int(w[0]), float(w[1]), int(w[2])) == (12 + r, 0.5 + 0.25 * r, ids[t])
                num = np.array([float(v) for v in w[3:]])
                assert _same_rows(num, got[r, t]), (r, t)
                assert "." not in w[6] and "." not in w[7]
        # the twin never touched the tracks: the fields are the same bits
        fa, fb = a.fields(), b.fields()
        for name in pkg.FIELDS:
            assert _bits_equal(fa[name], fb[name]), name


def test_a_tagged_particle_that_gets_lost_keeps_its_image_counts(pkg, fields):
    dims = S.SHAPES["O"]
    nx, ny, nz = dims
    p = _params(pkg, dims)
    f = dict(fields["O"])
    ux = np.full((nz, ny, nx), 2.0 * T.U_SCALE)   # everybody drifts along +x and wraps
    s_h = T.substep(p, cells=3.0) / 2.0           # 3 cells per substep
    n = 1000
    x, y, z = T.special_cloud(dims, n, 110)
    x[5], y[5], z[5] = nx - 2.5, 10.5, 2.5        # wraps in the first advance, meets the Inf in the second
    with pkg.Solver(p) as s:
        s.set_fields(f)
        s.set_field("ux", ux)
        s.set_field("uy", np.zeros_like(ux))
        s.set_field("uz", np.zeros_like(ux))
        s.tracers_set(x, y, z)
        s.tracks_arm(ids=[5, 6], values=["T"], capacity=4)
        s.tracers_advance(s_h, nsub=1)
        s.tracks_record(1, 0.0)
        x1, _, _, wx1, _ = s.tracers_get()
        assert wx1[5] == 1 and 0.25 < x1[5] < 0.75   # (the set-up: about 0.5, between the nodes 0 and 1)
        bad = ux.copy()
        bad[2, 10, 0] = np.inf
        s.set_field("ux", bad)
        s.tracers_advance(s_h, nsub=1)
        s.tracks_record(2, 1.0)
        _, _, rows = s.tracks_read()
        xs, ys, zs, wx, wy = s.tracers_get()
        assert np.isnan(xs[5]) and wx[5] == 1
        assert not np.isnan(rows[0, 0]).any() and rows[0, 0, 3] == 1.0
        assert np.isnan(rows[1, 0, :3]).all() and np.isnan(rows[1, 0, 5]) and rows[1, 0, 3] == 1.0 and rows[1, 0, 4] == float(wy[5])
        assert _same_rows(rows[1, 1], np.array([xs[6], ys[6], zs[6], wx[6], wy[6], s.tracers_sample("T")[0, 6]]))


# ---- 5. the run is left alone --------------------------------------------------------------------------------------------

def test_the_run_is_left_alone_and_release_gives_everything_back(pkg, tmp_path):
    dims = S.SHAPES["R"]
    p = _params(pkg, dims)
    n = 4097
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        for s in (a, b):
            _seeded_start(pkg, s)
            s.step(5)
        state, before = a.graph_state(), a.device_bytes()
        for call, msg in ((lambda: a.tracers_sample(["T"]), "tracers: no cloud"), (lambda: a.tracks_arm(ids=[0]), "tracers: no cloud"),
                          (lambda: a.tracks_record(1, 0.0), "ekpnp_tracks_record: no ring armed"), (lambda: a.tracks_save(str(tmp_path / "none.dat")), "no ring was armed")):
            with pytest.raises(pkg.EkpnpError) as e:
                call()
            assert msg in str(e.value) and "status 1" in str(e.value)
        assert a.tracks_count() == (0, 0) and not (tmp_path / "none.dat").exists()
        a.tracers_seed(n=n, seed=1)
        cloud = 56 * n + (2 + 1) * 12 * 8
        assert a.device_bytes() == before + cloud
        a.tracks_arm(ids=[4096, 0, 17], values=["T", "q"], capacity=4)
        ring = 48 + 4 * 3 * 7 * 8   # four tables of three int32 (a multiple of 16 bytes), four rows of [3][7] doubles
        assert a.device_bytes() == before + cloud + ring
        for k in range(6):
            a.step(1)
            b.step(1)
            a.tracers_advance(p.dt, nsub=1)
            a.tracks_record(k, a.t)
            got = a.tracers_sample(["T", "uz"] if k < 3 else ["T", "uz", "c", "q"])
            assert got.shape[1] == n
            assert a.device_bytes() == before + cloud + ring + (2 if k < 3 else 4) * n * 8   # the scratch grows on demand, and only then
        assert a.graph_state() == state and b.graph_state() == state and a.tracks_count() == (6, 2)
        fa, fb = a.fields(), b.fields()
        for name in pkg.FIELDS:
            assert _bits_equal(fa[name], fb[name]), name
        # seed, set and load disarm the tracks; the rows stay readable
        x, y, z, _, _ = a.tracers_get()
        a.tracers_save(str(tmp_path / "cloud.bin"))
        for replace in (lambda: a.tracers_seed(n=n, seed=2), lambda: a.tracers_set(x, y, z), lambda: a.tracers_load(str(tmp_path / "cloud.bin"))):
            a.tracks_arm(ids=[1, 0], capacity=2)
            a.tracks_record(7, 0.0)
            replace()
            with pytest.raises(pkg.EkpnpError) as e:
                a.tracks_record(8, 0.0)
            assert "ekpnp_tracks_record: no ring armed" in str(e.value)
            assert a.tracks_count() == (1, 0) and a.tracks_read()[2].shape == (1, 2, 5)
        a.tracks_disarm()
        with pytest.raises(pkg.EkpnpError) as e:
            a.tracks_arm(ids=[n], capacity=2)
        assert f"id {n}" in str(e.value)
        with pytest.raises(pkg.EkpnpError) as e:
            a.tracks_arm(ids=[1], capacity=0)
        assert "capacity = 0" in str(e.value)
        with pytest.raises(pkg.EkpnpError) as e:
            a.tracers_sample(["T", "T"])
        assert "named twice" in str(e.value)
        a.tracers_release()
        assert a.device_bytes() == before and a.tracks_count() == (0, 0)


def test_slab_contexts_and_groups_are_refused(pkg):
    import ctypes as C

    p = _params(pkg, S.SHAPES["W"])
    L = pkg.load_library()
    ids = np.array([0], dtype=np.int32)
    out = np.zeros(8)
    lab = np.zeros(1, dtype=np.int64)
    spec = pkg.tracks_spec(ids=[0])
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)

    def raw_calls(h):
        r, d = C.c_int64(), C.c_int64()
        return [L.ekpnp_tracers_sample(h, 1, ptr(ids), ptr(out)), L.ekpnp_tracers_sample_device(h, 1, ptr(ids), ptr(out)),
                L.ekpnp_tracks_arm(h, C.byref(spec), 1), L.ekpnp_tracks_disarm(h), L.ekpnp_tracks_record(h, 1, 0.0),
                L.ekpnp_tracks_count(h, C.byref(r), C.byref(d)), L.ekpnp_tracks_read(h, 0, 0, ptr(lab), ptr(out), ptr(out)),
                L.ekpnp_tracks_save(h, b"unused.dat")]

    for rank, nranks in ((0, 1), (1, 3)):
        with pkg.Solver(p, rank=rank, nranks=nranks, slab=True) as s:
            calls = [lambda: s.tracers_sample(["T"]), lambda: s.tracers_sample_into(["T"], 8), lambda: s.tracks_arm(ids=[0]), lambda: s.tracks_disarm(),
                     lambda: s.tracks_record(1, 0.0), lambda: s.tracks_count(), lambda: s.tracks_read(0, 0), lambda: s.tracks_save("unused.dat")]
            for k, call in enumerate(calls):
                with pytest.raises(pkg.EkpnpError) as e:
                    call()
                assert "status 1" in str(e.value) and SLAB_MSG in str(e.value), k
    with pkg.Group(p, 2, devices=[0, 0]) as g:
        for i in range(2):
            h = g.slab_handle(i)
            for k, rc in enumerate(raw_calls(h)):
                assert rc == 1 and SLAB_MSG.encode() in L.ekpnp_last_error(h), (i, k)
    assert not os.path.exists("unused.dat")


# ---- 6. the driver ---------------------------------------------------------------------------------------------------

GEO = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "8", "--seed-pattern", "squares", "--seed-modes", "1,1"]


def _run_driver(args, out, code=0):
    out.mkdir()
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1", EKPNP_PLACEMENT_TRIES="1")  # the child shares device 0 with this process
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == code, (args, r.returncode, r.stderr[-2000:])
    return out, r.stderr


def test_driver_writes_the_tracks_the_library_calls_give(pkg, tmp_path):
    assert os.path.exists(EXE), "ekpnp_main not built"
    flags = ["--tracers-grid", "8,8,4", "--tracks-first", "5", "--tracks-values", "T,q", "--tracks-every", "2"]
    loop, _ = _run_driver([*GEO, *flags], tmp_path / "loop")
    batch, _ = _run_driver([*GEO, *flags, "--batch", "1"], tmp_path / "batch")
    plain, _ = _run_driver([*GEO, "--tracers-grid", "8,8,4"], tmp_path / "plain")
    assert sorted(os.listdir(loop)) == sorted(os.listdir(batch)) == sorted(os.listdir(plain) + ["tracks.dat"])
    for f in os.listdir(loop):
        assert (loop / f).read_bytes() == (batch / f).read_bytes(), f
        if f != "tracks.dat":
            assert (loop / f).read_bytes() == (plain / f).read_bytes(), f
    # the same run through the library: seeded start, a step and an advance per iteration, a row after every second
    p = pkg.default_params(40, 12, 17)
    seed = pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-3, noise=0.0, relative=True, seed=1)
    want = tmp_path / "want.dat"
    with pkg.Solver(p) as s:
        s.initialization()
        s.seed(seed)
        s.fast_Poisson()
        s.init_equilibrium()
        s.tracers_seed(grid=(8, 8, 4))
        s.tracks_arm(ids=range(5), values=["T", "q"], capacity=4)
        t = 0.0
        for i in range(8):
            s.stream_collide_save(t)
            s.fast_Poisson()
            t = t + p.dt
            s.tracers_advance(p.dt, nsub=1)
            if (i + 1) % 2 == 0:
                s.tracks_record(i + 1, t)
        s.tracks_save(str(want))
    assert (loop / "tracks.dat").read_bytes() == want.read_bytes()
    lines = want.read_text().splitlines()
    assert lines[0] == "# ekpnp tracks nx 40 ny 12 nz 17 n 256 ntags 5 nvalues 2 recorded 4 dropped 0" and lines[1].endswith("wx wy T q") and len(lines) == 2 + 4 * 5
    # explicit ids, no values
    ids, _ = _run_driver([*GEO, "--tracers-grid", "8,8,4", "--tracks", "255,0,17"], tmp_path / "ids")
    lines = (ids / "tracks.dat").read_text().splitlines()
    assert len(lines) == 2 + 8 * 3 and [ln.split(" ")[2] for ln in lines[2:5]] == ["255", "0", "17"] and len(lines[2].split(" ")) == 8
    for bad, number in ((["--tracks-first", "5"], "there is no cloud to tag"), (["--tracks-values", "T"], "there is no cloud to tag"),
                        (["--tracers", "10", "--tracks-every", "2"], "no particle is tagged"), (["--tracers", "10", "--tracks", "3,10"], "id 10"),
                        (["--tracers", "10", "--tracks", "3,3"], "id 3 is tagged twice"), (["--tracers", "10", "--tracks", "3,x"], "got 3,x"),
                        (["--tracers", "10", "--tracks-first", "0"], "got 0"), (["--tracers", "10", "--tracks-first", "2", "--tracks-values", "T,w"], "got w in T,w"),
                        (["--tracers", "10", "--tracks-first", "2", "--tracks-values", "T,T"], "named twice"),
                        (["--tracers", "10", "--tracks-first", "2", "--tracks-every", "0"], "got 0"),
                        (["--tracers", "10", "--tracks-first", "2", "--gpus", "2", "--devices", "0,0"], "slab contexts are not supported")):
        _, err = _run_driver([*GEO, *bad], tmp_path / ("bad" + "_".join(bad).replace("-", "").replace(",", "_")), code=2)
        assert number in err, err
