"""GPU tests of the per-step scalar time series (csrc/monitor.hip; include/ekpnp.h: ekpnp_monitor_* and the
ekpnp_group_monitor_* spellings; `ekpnp_main --monitor-every N`).

The rows an armed monitor appends from inside step() - through the replayed step graph too - are held bit for bit against the
synchronous values of a twin that stops after every step (monitor_sample, current(), umax()); the sums are held against exact
host sums of the get_field arrays, with a bound that is derived, not measured: for a sum over n terms
|gpu - exact| <= (n + 8) * 2**-53 * fsum(|term| magnitudes), the first-order bound for ANY order of n additions plus a few
roundings per term, the magnitude of a composite term being the product or sum of the absolute values of its operands."""
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
SHAPE = (40, 12, 17)
SUMS = (0, 1, 2, 3, 5, 6, 7, 8)  # the columns that are sums of many terms


def _mirror(pkg, po):
    p = pkg.Params()
    for name, _ in p._fields_:
        setattr(p, name, getattr(po, name))
    return p


def _perturbed_params(pkg, O, shape, in_place=0):
    po = O.default_params(*shape)
    po.pb_iterations = 20
    p = _mirror(pkg, po)
    p.in_place = in_place
    return po, p


def _perturbed_run(pkg, O, shape, steps, in_place=0, **knobs):
    """the perturbed start of tests/test_io_gpu.py on the library's own initialization, then `steps` steps"""
    po, p = _perturbed_params(pkg, O, shape, in_place)
    s = pkg.Solver(p)
    for k, v in knobs.items():
        s.tune(k, v)
    s.initialization()
    s.set_fields(O.perturb_fields(po, s.fields()))
    s.fast_Poisson()
    s.init_equilibrium()
    if steps:
        s.step(steps)
    return s


def _perturbed_group(pkg, O, shape, nslabs):
    po, p = _perturbed_params(pkg, O, shape)
    g = pkg.Group(p, nslabs, devices=[0] * nslabs)
    g.initialization()
    g.set_fields(O.perturb_fields(po, g.fields()))
    g.fast_Poisson()
    g.init_equilibrium()
    return g


def _random_fields(pkg, shape_zyx, seed):
    rng = np.random.default_rng(seed)
    scale = {"rho": 1000.0, "c": 30.0, "cn": 30.0, "phi": 5e-3, "T": 1.0, "Ex": 1e5, "Ey": 1e5, "Ez": 1e5}
    return {n: scale.get(n, 1e-3) * rng.uniform(-1.0, 1.0, size=shape_zyx) for n in pkg.FIELDS}


def _plate_terms(f, top, bottom):
    """{column: (terms, magnitudes)} of the plate sums the planes of `f` hold; f is [nz_local][ny][nx]"""
    out = {}
    a = np.abs
    if top:
        c1, c2, n1, n2, e = f["c"][-2], f["c"][-3], f["cn"][-2], f["cn"][-3], f["Ez"][-1]
        out[0] = (((2.0 * c1 - c2) - (2.0 * n1 - n2)) * e, (2 * a(c1) + a(c2) + 2 * a(n1) + a(n2)) * a(e))
        t0, t1, t2 = f["T"][-1], f["T"][-2], f["T"][-3]
        out[3] = (3.0 * t0 - 4.0 * t1 + t2, 3 * a(t0) + 4 * a(t1) + a(t2))
    if bottom:
        c1, c2, n1, n2, e = f["c"][1], f["c"][2], f["cn"][1], f["cn"][2], f["Ez"][0]
        out[1] = (((2.0 * c1 - c2) - (2.0 * n1 - n2)) * e, (2 * a(c1) + a(c2) + 2 * a(n1) + a(n2)) * a(e))
        t0, t1, t2 = f["T"][0], f["T"][1], f["T"][2]
        out[2] = (4.0 * t1 - 3.0 * t0 - t2, 4 * a(t1) + 3 * a(t0) + a(t2))
    return out


def _volume_terms(f):
    a = np.abs
    q, qm = f["c"] - f["cn"], a(f["c"]) + a(f["cn"])
    uu = f["ux"] * f["ux"] + f["uy"] * f["uy"] + f["uz"] * f["uz"]
    return {5: (uu, uu), 6: (q, qm), 7: (q * q, qm * qm), 8: (f["uz"] * f["T"], a(f["uz"]) * a(f["T"]))}


def _check_against_exact_sums(pkg, got, f, p, tag, top=True, bottom=True):
    """|gpu - exact| <= (n + 8) * 2**-53 * fsum(magnitudes) for the sums; the maxima and the count exactly"""
    scale = p.K * p.dz * p.dz
    terms = {**_plate_terms(f, top, bottom), **_volume_terms(f)}
    worst = 0.0
    for col in SUMS:
        if col not in terms:
            assert got[col] == 0.0 and not np.signbit(got[col]), (tag, pkg.MONITOR_NAMES[col], got[col])
            continue
        t, m = (v.ravel().tolist() for v in terms[col])
        exact, bound = math.fsum(t), (len(t) + 8) * 2.0 ** -53 * math.fsum(m)
        if col in (0, 1):
            exact, bound = exact * scale, bound * scale
        err = abs(got[col] - exact)
        if bound > 0.0:
            worst = max(worst, err / bound)
        assert err <= bound, (tag, pkg.MONITOR_NAMES[col], got[col], exact, err, bound)
    assert got[4] == max(0.0, f["uz"].max()), (tag, got[4])
    assert got[9] == np.abs(f["rho"] - p.rho0).max(), (tag, got[9])
    assert got[10] == 0.0, (tag, got[10])
    print(f"{tag}: largest |gpu - exact| / bound = {worst:.3e}")


# ---- 1. the series equals the synchronous values, through the graph --------------------------------------

@pytest.fixture(scope="module")
def series(pkg, O):
    """Context A: armed with all quantities, every = 1, then ONE step(9) (one eager step out of the equilibrium start, four
    replays of the captured pair).  Twin B: nine times step(1) and the synchronous calls.  Shared by the tests below, unchanged."""
    with _perturbed_run(pkg, O, SHAPE, 0) as a, _perturbed_run(pkg, O, SHAPE, 0) as b:
        a.monitor_arm(None, every=1, capacity=64)
        a.step(9)
        graph = a.graph_state()
        count = a.monitor_count()
        steps, times, values = a.monitor_read()
        rows, t, cur, um = [], [], [], []
        for _ in range(9):
            b.step(1)
            rows.append(b.monitor_sample())
            cur.append(b.current())
            um.append(b.umax())
            t.append(b.t)
        fa, fb = a.fields(), b.fields()
    return dict(graph=graph, count=count, steps=steps, times=times, values=values, rows=np.array(rows), t=np.array(t),
                current=np.array(cur), umax=np.array(um), fa=fa, fb=fb)


def test_series_equals_the_synchronous_values_through_the_graph(pkg, series):
    s = series
    assert s["graph"] == 1  # under 4 M nodes and nsteps >= 4: the replay path
    assert s["count"] == (9, 0)
    assert s["steps"].tolist() == list(range(1, 10))
    assert np.array_equal(s["times"], s["t"])
    assert s["values"].shape == (9, 11)
    assert np.array_equal(s["values"], s["rows"]), np.argwhere(s["values"] != s["rows"])[:5]
    assert np.array_equal(s["values"][:, pkg.MONITOR_ID["current_top"]], s["current"])
    assert np.array_equal(s["values"][:, pkg.MONITOR_ID["uz_max"]], s["umax"])
    for name in pkg.FIELDS:  # recording does not disturb the run
        assert np.array_equal(s["fa"][name], s["fb"][name]), name
    for name in ("current_top", "u_u", "uz_max"):  # the run has structure
        assert (s["values"][:, pkg.MONITOR_ID[name]] != 0.0).all(), name
    assert not np.array_equal(s["values"][0], s["values"][8])


# ---- 2. every way of stepping gives the same bits --------------------------------------------------------

MODES = [
    ("in_place", dict(in_place=1), 1, (9,)),
    ("batch_moments", dict(batch_moments=1), 1, (9,)),
    ("batch_moments", dict(batch_moments=1), 3, (9,)),
    ("eager_efield", dict(lazy_efield=0), 1, (9,)),
    ("cut", dict(), 1, (5, 1, 3)),
    ("cut", dict(), 3, (5, 1, 3)),
    ("cut_batch_moments", dict(batch_moments=1), 3, (5, 1, 3)),
    ("kernel_timing", dict(), 1, (9,)),
]


@pytest.mark.parametrize("tag, knobs, every, cuts", MODES, ids=[f"{m[0]}-every{m[2]}" for m in MODES])
def test_modes_give_the_same_bits(pkg, O, series, tag, knobs, every, cuts):
    with _perturbed_run(pkg, O, SHAPE, 0, **knobs) as s:
        if tag == "kernel_timing":
            s.kernel_timing(True)
        s.monitor_arm(None, every=every, capacity=64)
        for n in cuts:
            s.step(n)
        steps, times, values = s.monitor_read()
        f = s.fields()
    want = [k for k in range(1, 10) if k % every == 0]
    assert steps.tolist() == want
    idx = [k - 1 for k in want]
    assert np.array_equal(times, series["times"][idx])
    assert np.array_equal(values, series["values"][idx]), np.argwhere(values != series["values"][idx])[:5]
    for name in pkg.FIELDS:
        assert np.array_equal(f[name], series["fa"][name]), name


# ---- 3. against exact host sums --------------------------------------------------------------------------

def test_sample_of_a_running_lattice_against_exact_sums(pkg, O):
    with _perturbed_run(pkg, O, SHAPE, 12) as s:
        got = s.monitor_sample()  # right after a lazy solve: nothing has looked at E
        again = s.monitor_sample()
        f = s.fields()
        after = s.monitor_sample()  # now from the Ez array
        p = s.p
    assert np.array_equal(got, again) and np.array_equal(got, after)
    _check_against_exact_sums(pkg, got, f, p, "40x12x17")


def test_sample_of_a_plane_of_several_workgroups_against_exact_sums(pkg):
    """200 x 96 = 19 200 nodes per plane: several workgroups of the volume pass's 4 096-node runs, the last partly filled, and
    more than one stride of the plate pass; seeded fields of mixed sign, no stepping."""
    p = pkg.default_params(200, 96, 8)
    with pkg.Solver(p) as s:
        s.set_fields(_random_fields(pkg, s.shape, 11))
        got = s.monitor_sample()
        f = s.fields()
    _check_against_exact_sums(pkg, got, f, p, "200x96x8")


# ---- 4. exact known answer -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["z_only", "xy"])
def test_small_integer_fields_give_the_integers_exactly(pkg, case):
    nx, ny, nz = 50, 8, 9
    p = pkg.default_params(nx, ny, nz)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    fi = {}
    for k, name in enumerate(pkg.FIELDS):  # small integers of both signs, a different pattern per field
        if case == "z_only":
            fi[name] = ((k + 2) * z - 3 * k + 1).astype(np.int64)
        else:
            fi[name] = (((k + 1) * x + (2 * k + 3) * y) % 7 - 3 + z * (k % 3)).astype(np.int64)
    with pkg.Solver(p) as s:
        s.set_fields({n: v.astype(np.float64) for n, v in fi.items()})
        got = s.monitor_sample()
    c, cn, T, ez = fi["c"], fi["cn"], fi["T"], fi["Ez"]
    q = c - cn
    i_top = int((((2 * c[-2] - c[-3]) - (2 * cn[-2] - cn[-3])) * ez[-1]).sum())
    i_bot = int((((2 * c[1] - c[2]) - (2 * cn[1] - cn[2])) * ez[0]).sum())
    want = {
        0: float(i_top) * p.K * p.dz * p.dz,
        1: float(i_bot) * p.K * p.dz * p.dz,
        2: float((4 * T[1] - 3 * T[0] - T[2]).sum()),
        3: float((3 * T[-1] - 4 * T[-2] + T[-3]).sum()),
        4: float(max(0, fi["uz"].max())),
        5: float((fi["ux"] ** 2 + fi["uy"] ** 2 + fi["uz"] ** 2).sum()),
        6: float(q.sum()),
        7: float((q * q).sum()),
        8: float((fi["uz"] * T).sum()),
        9: float(np.abs(fi["rho"].astype(np.float64) - p.rho0).max()),
        10: 0.0,
    }
    for col in range(11):
        assert got[col] == want[col], (pkg.MONITOR_NAMES[col], got[col], want[col])


# ---- 5. NaN and Inf --------------------------------------------------------------------------------------

def test_nonfinite_nodes_are_counted_and_do_not_reach_rho_dev(pkg):
    p = pkg.default_params(50, 8, 9)
    with pkg.Solver(p) as s:
        f = _random_fields(pkg, s.shape, 7)
        f["rho"][2, 3, 4] = np.nan
        f["T"][5, 1, 7] = np.inf
        f["c"][1, 2, 3] = np.nan
        f["cn"][1, 2, 3] = np.inf
        s.set_fields(f)
        got = s.monitor_sample()
    assert got[pkg.MONITOR_ID["nonfinite"]] == 3.0
    dev = np.abs(f["rho"] - p.rho0)
    assert np.isfinite(got[pkg.MONITOR_ID["rho_dev"]]) and got[pkg.MONITOR_ID["rho_dev"]] == np.nanmax(dev)
    assert got[pkg.MONITOR_ID["uz_max"]] == max(0.0, f["uz"].max())


# ---- 6. the ring -----------------------------------------------------------------------------------------

def test_ring_overwrites_the_oldest_rows_and_counts_them(pkg, O, series):
    with _perturbed_run(pkg, O, SHAPE, 0) as s, _perturbed_run(pkg, O, SHAPE, 0) as big:
        unarmed = s.device_bytes()
        assert big.device_bytes() == unarmed
        s.monitor_arm(None, every=1, capacity=4)
        big.monitor_arm(None, every=1, capacity=64)  # the uncut twin with room for every row
        armed = s.device_bytes()
        assert armed > unarmed  # ring, scratch and cursor are counted ...
        assert s.monitor_count() == (0, 0)
        s.step(10)
        big.step(10)
        assert s.monitor_count() == (10, 6) and big.monitor_count() == (10, 0)
        steps, times, values = s.monitor_read(0, 4)
        s64, t64, v64 = big.monitor_read()
        assert steps.tolist() == [7, 8, 9, 10] and s64.tolist() == list(range(1, 11))
        assert np.array_equal(values, v64[6:]) and np.array_equal(times, t64[6:])
        assert np.array_equal(v64[:9], series["values"])
        assert np.array_equal(values[3], s.monitor_sample()) and times[3] == s.t
        one = s.monitor_read(2, 1)
        assert one[0].tolist() == [9] and np.array_equal(one[2][0], series["values"][8])
        with pytest.raises(pkg.EkpnpError):
            s.monitor_read(0, 5)
        with pytest.raises(pkg.EkpnpError):
            s.monitor_read(-1, 1)
        s.monitor_arm(None, every=1, capacity=4)
        assert s.monitor_count() == (0, 0)
        assert s.device_bytes() == armed  # ... and allocated once
        s.step(2)
        assert s.monitor_read()[0].tolist() == [1, 2]
        s.monitor_disarm()
        s.step(4)
        assert s.monitor_count() == (2, 0)  # nothing is appended any more; the rows stay readable
    with _perturbed_run(pkg, O, SHAPE, 0) as s:  # a context that never arms allocates nothing for it
        assert s.device_bytes() == unarmed
        s.step(4)
        assert s.device_bytes() == unarmed and s.monitor_count() == (0, 0)
        with pytest.raises(pkg.EkpnpError):
            s.monitor_record(1, 0.0)


# ---- 7. plates only --------------------------------------------------------------------------------------

def test_plates_only_leaves_the_other_columns_zero(pkg, O, series):
    with _perturbed_run(pkg, O, SHAPE, 0) as s:
        s.monitor_arm([0, 1, 2, 3], every=1, capacity=16)
        s.step(9)
        steps, times, values = s.monitor_read()
        now = s.monitor_sample(["current_top", "current_bottom", "dTdz_bottom", "dTdz_top"])
    assert steps.tolist() == list(range(1, 10))
    assert (values[:, 4:] == 0.0).all() and not np.signbit(values[:, 4:]).any()
    assert np.array_equal(values[:, :4], series["values"][:, :4])
    assert np.array_equal(now, values[8])


# ---- 8. groups -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nslabs", [2, 3])
def test_group_series_equals_the_synchronous_values(pkg, O, nslabs):
    with _perturbed_group(pkg, O, SHAPE, nslabs) as a, _perturbed_group(pkg, O, SHAPE, nslabs) as b:
        a.monitor_arm(None, every=1, capacity=16)
        a.step(6)
        assert a.monitor_count() == (6, 0)
        steps, times, values = a.monitor_read()
        rows, t, cur, um = [], [], [], []
        for _ in range(6):
            b.step(1)
            rows.append(b.monitor_sample())
            cur.append(b.current())
            um.append(b.umax())
            t.append(b.t)
        f = b.fields()
        p = b.p
        with pytest.raises(pkg.EkpnpError):
            a.monitor_read(0, 7)
        assert a.monitor_read(5, 1)[0].tolist() == [6]  # a refused range leaves the group usable
    assert steps.tolist() == [1, 2, 3, 4, 5, 6] and np.array_equal(times, np.array(t))
    assert np.array_equal(values, np.array(rows))
    assert np.array_equal(values[:, 0], np.array(cur)) and np.array_equal(values[:, 4], np.array(um))
    assert (values[:, 0] != 0.0).all() and (values[:, 5] != 0.0).all()
    _check_against_exact_sums(pkg, values[5], f, p, f"40x12x17 in {nslabs} slabs")


def test_slab_without_a_plate_contributes_plus_zero(pkg):
    p = pkg.default_params(*SHAPE)
    with pkg.Solver(p, rank=1, nranks=3, slab=True) as s:
        assert s.z0 > 0 and s.z0 + s.nz_local < p.nz
        s.set_fields(_random_fields(pkg, s.shape, 3))
        got = s.monitor_sample()
        f = s.fields()
    _check_against_exact_sums(pkg, got, f, p, "slab 1 of 3", top=False, bottom=False)


# ---- 9. record and the file ------------------------------------------------------------------------------

def _read_monitor(path):
    lines = open(path).read().splitlines()
    h = lines[0].split(" ")
    assert h[:3] == ["#", "ekpnp", "monitor"] and h[3::2] == ["nx", "ny", "nz", "every", "recorded", "dropped"], lines[0]
    hdr = {k: int(v) for k, v in zip(h[3::2], h[4::2])}
    names = lines[1].split(" ")
    assert names[:3] == ["#", "step", "time"]
    rows = [ln.split(" ") for ln in lines[2:]]
    assert all(len(r) == 2 + 11 for r in rows)
    steps = [int(r[0]) for r in rows]
    data = np.array([[float(v) for v in r[1:]] for r in rows]).reshape(len(rows), 12)
    return hdr, names[3:], steps, data[:, 0], data[:, 1:]


def test_record_with_the_callers_labels_and_the_file(pkg, O, series, tmp_path):
    with _perturbed_run(pkg, O, SHAPE, 0) as s:
        s.monitor_arm(None, every=1000, capacity=8)  # armed, but no automatic row falls into these steps
        for k in range(1, 6):
            s.step(1)
            s.monitor_record(k, s.t)
        assert s.monitor_count() == (5, 0)
        steps, times, values = s.monitor_read()
        assert steps.tolist() == [1, 2, 3, 4, 5]
        assert np.array_equal(times, series["times"][:5]) and np.array_equal(values, series["values"][:5])
        s.monitor_save(str(tmp_path / "m.dat"))
        hdr, names, fsteps, ftimes, fvalues = _read_monitor(tmp_path / "m.dat")
        assert hdr == dict(nx=40, ny=12, nz=17, every=1000, recorded=5, dropped=0)
        assert names == pkg.MONITOR_NAMES and fsteps == [1, 2, 3, 4, 5]
        assert np.array_equal(ftimes, times) and np.array_equal(fvalues, values)  # %.17g round-trips
        with pytest.raises(pkg.EkpnpError):
            s.monitor_save(str(tmp_path / "no_such_directory" / "m.dat"))
        s.step(1)  # the context stays usable
        s.monitor_record(6, s.t)
        assert np.array_equal(s.monitor_read(5, 1)[2][0], series["values"][5])
    with _perturbed_group(pkg, O, SHAPE, 2) as g:
        g.monitor_arm(None, every=2, capacity=2)
        g.step(6)
        assert g.monitor_count() == (3, 1)
        steps, times, values = g.monitor_read()
        g.monitor_save(str(tmp_path / "g.dat"))
        hdr, names, fsteps, ftimes, fvalues = _read_monitor(tmp_path / "g.dat")
        assert hdr == dict(nx=40, ny=12, nz=17, every=2, recorded=3, dropped=1)
        assert fsteps == steps.tolist() == [4, 6] and np.array_equal(fvalues, values) and np.array_equal(ftimes, times)
        assert np.array_equal(values[1], g.monitor_sample())
        with pytest.raises(pkg.EkpnpError):
            g.monitor_save(str(tmp_path / "no_such_directory" / "g.dat"))
        g.step(1)


# ---- 10. the driver --------------------------------------------------------------------------------------

def _run_driver(args, out):
    out.mkdir()
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1", EKPNP_PLACEMENT_TRIES="1")  # the child shares device 0 with this process
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (args, r.stderr[-2000:])
    return out


def test_driver_writes_the_same_series_from_either_loop(pkg, tmp_path):
    """The monitor changes no other file.  A three-slab run is held against a three-slab run WITHOUT the monitor: a slab run's
    data.dat differs from a single context's in a last printed digit to begin with (the slab z solve eliminates in another
    order; tests/test_group_gpu.py holds the two to 1e-9), monitor or not."""
    assert os.path.exists(EXE), "ekpnp_main not built"
    geo = ["--nx", "40", "--ny", "6", "--nz", "33", "--steps", "47", "--nsave", "15", "--print-current", "10", "--uw", "3e-4"]
    plain = _run_driver(geo, tmp_path / "plain")
    loop = _run_driver([*geo, "--monitor-every", "4"], tmp_path / "loop")
    batch = _run_driver([*geo, "--monitor-every", "4", "--batch", "1"], tmp_path / "batch")
    slabs = _run_driver([*geo, "--monitor-every", "4", "--batch", "1", "--devices", "0,0,0"], tmp_path / "slabs")
    assert not (plain / "monitor.dat").exists()
    hdr, names, steps, times, values = _read_monitor(loop / "monitor.dat")
    assert hdr == dict(nx=40, ny=6, nz=33, every=4, recorded=11, dropped=0)
    assert names == pkg.MONITOR_NAMES and steps == list(range(4, 45, 4))
    assert np.isfinite(values).all() and (values[:, 10] == 0.0).all() and (values[:, 0] != 0.0).all()
    assert (loop / "monitor.dat").read_bytes() == (batch / "monitor.dat").read_bytes()
    ghdr, _, gsteps, gtimes, gvalues = _read_monitor(slabs / "monitor.dat")
    assert ghdr == hdr and gsteps == steps and np.array_equal(gtimes, times)
    for f in ("data.dat", "umax.dat", "data_end.dat"):
        a = (plain / f).read_bytes()
        assert len(a) > 0 and a == (loop / f).read_bytes() and a == (batch / f).read_bytes(), f
    plain_slabs = _run_driver([*geo, "--devices", "0,0,0"], tmp_path / "plain_slabs")
    for f in ("data.dat", "umax.dat", "data_end.dat"):
        a = (plain_slabs / f).read_bytes()
        assert len(a) > 0 and a == (slabs / f).read_bytes(), f
