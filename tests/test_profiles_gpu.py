"""GPU tests of the on-device plane profiles and running statistics (csrc/stats.hip; include/ekpnp.h: ekpnp_plane_sums,
ekpnp_stats_*, ekpnp_save_profiles and the ekpnp_group_* spellings; `ekpnp_main --profiles-every N`).

The 24 sums of a plane are checked against sums formed on the host from the get_field arrays (terms in float64 with numpy,
each plane added exactly with math.fsum), against integer arithmetic where every sum is exactly representable, and for the
property the reduction is built around: the bits of a plane's sums do not depend on how the lattice is held or cut."""
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")


def _mirror(pkg, po):
    p = pkg.Params()
    for name, _ in p._fields_:
        setattr(p, name, getattr(po, name))
    return p


def _terms(pkg, f):
    """the 24 per-node terms in id order, float64, each product rounded once (numpy)"""
    q = f["c"] - f["cn"]
    t = [f[n] for n in pkg.FIELDS]
    t += [f["ux"] * f["ux"], f["uy"] * f["uy"], f["uz"] * f["uz"], f["c"] * f["c"], f["cn"] * f["cn"], f["T"] * f["T"]]
    t += [f["uz"] * f["T"], f["uz"] * f["c"], f["uz"] * f["cn"], q * f["Ex"], q * f["Ez"], f["ux"] * f["uz"], q * q]
    assert len(t) == len(pkg.PROFILE_NAMES)
    return t


def _check_against_exact_sums(pkg, got, f, tag):
    """|gpu - exact| <= 2 * nx*ny * 2**-53 * fsum(|terms|) per entry: any order of n floating-point additions errs by at most
    (n-1) u sum|term| to first order, and a fused multiply-add differs from numpy's rounded product by at most u per term."""
    nz, ny, nx = f["rho"].shape
    assert got.shape == (len(pkg.PROFILE_NAMES), nz)
    worst = 0.0
    for q, t in enumerate(_terms(pkg, f)):
        for z in range(nz):
            plane = t[z].ravel().tolist()
            exact, mag = math.fsum(plane), math.fsum(abs(v) for v in plane)
            bound = 2.0 * nx * ny * 2.0 ** -53 * mag
            err = abs(got[q, z] - exact)
            if bound > 0.0:
                worst = max(worst, err / bound)
            assert err <= bound, (tag, pkg.PROFILE_NAMES[q], z, got[q, z], exact, err, bound)
    print(f"{tag}: largest |gpu - exact| / bound = {worst:.3e}")


def _perturbed_run(pkg, O, shape, steps, **knobs):
    """the perturbed start of tests/test_io_gpu.py on the library's own initialization, then `steps` steps"""
    po = O.default_params(*shape)
    po.pb_iterations = 20
    s = pkg.Solver(_mirror(pkg, po))
    for k, v in knobs.items():
        s.tune(k, v)
    s.initialization()
    s.set_fields(O.perturb_fields(po, s.fields()))
    s.fast_Poisson()
    s.init_equilibrium()
    if steps:
        s.step(steps)
    return s


def _random_fields(pkg, shape_zyx, seed):
    rng = np.random.default_rng(seed)
    scale = {"rho": 1000.0, "c": 30.0, "cn": 30.0, "phi": 5e-3, "T": 1.0, "Ex": 1e5, "Ey": 1e5, "Ez": 1e5}
    return {n: scale.get(n, 1e-3) * rng.uniform(-1.0, 1.0, size=shape_zyx) for n in pkg.FIELDS}


# ---- 1. against exact sums ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(40, 12, 17), (50, 8, 51)])
def test_plane_sums_of_a_running_lattice_against_exact_sums(pkg, O, shape):
    with _perturbed_run(pkg, O, shape, 12) as s:
        got = s.plane_sums()
        f = s.fields()
    _check_against_exact_sums(pkg, got, f, "x".join(map(str, shape)))


def test_plane_sums_of_a_plane_of_several_workgroups_against_exact_sums(pkg):
    """200 x 96 = 19 200 nodes per plane: several workgroups of the kernel's 4 096-node runs and no multiple of them (nor of a
    larger power of two a re-tuned run length might be); seeded fields of mixed sign, no stepping."""
    p = pkg.default_params(200, 96, 8)
    with pkg.Solver(p) as s:
        s.set_fields(_random_fields(pkg, s.shape, 11))
        got = s.plane_sums()
        f = s.fields()
    _check_against_exact_sums(pkg, got, f, "200x96x8")


# ---- 2. exact known answer ---------------------------------------------------------------------------

def _integer_terms(fi):
    q = fi["c"] - fi["cn"]
    names = ["rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T"]
    t = [fi[n] for n in names]
    t += [fi["ux"] * fi["ux"], fi["uy"] * fi["uy"], fi["uz"] * fi["uz"], fi["c"] * fi["c"], fi["cn"] * fi["cn"], fi["T"] * fi["T"]]
    t += [fi["uz"] * fi["T"], fi["uz"] * fi["c"], fi["uz"] * fi["cn"], q * fi["Ex"], q * fi["Ez"], fi["ux"] * fi["uz"], q * q]
    return t


@pytest.mark.parametrize("case", ["z_only", "xy"])
def test_small_integer_fields_give_the_integer_sums_exactly(pkg, case):
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
        got = s.plane_sums()
    want = np.array([[int(t[zz].sum()) for zz in range(nz)] for t in _integer_terms(fi)], dtype=np.int64)
    assert np.abs(want).max() < 2 ** 40
    assert got.shape == want.shape
    assert (got == want.astype(np.float64)).all(), np.argwhere(got != want)[:5]


# ---- 3. independent of the decomposition -------------------------------------------------------------

def test_plane_sums_do_not_depend_on_the_decomposition(pkg):
    nx, ny, nz = 96, 50, 19  # 4 800 nodes per plane: two workgroups, the second one partly filled
    p = pkg.default_params(nx, ny, nz)
    f = _random_fields(pkg, (nz, ny, nx), 5)
    with pkg.Solver(p) as s:
        s.set_fields(f)
        ref = s.plane_sums()
        again = s.plane_sums()
    assert np.array_equal(ref, again)
    _check_against_exact_sums(pkg, ref, f, "96x50x19")
    pi = p.copy()
    pi.in_place = 1
    with pkg.Solver(pi) as s:
        s.set_fields(f)
        assert np.array_equal(s.plane_sums(), ref)
    for nslabs in (2, 3):
        with pkg.Group(p, nslabs, devices=[0] * nslabs) as g:
            if nslabs == 3:
                assert [g.slab_extent(i)[1] for i in range(3)] == [6, 6, 7]
            g.set_fields(f)
            assert np.array_equal(g.plane_sums(), ref), nslabs
    for rank in range(3):
        with pkg.Solver(p, rank=rank, nranks=3, slab=True) as s:
            z0, nzl = s.z0, s.nz_local
            s.set_fields({n: v[z0:z0 + nzl] for n, v in f.items()})
            assert np.array_equal(s.plane_sums(), ref[:, z0:z0 + nzl]), rank


# ---- 4. accumulation -----------------------------------------------------------------------------------

@pytest.mark.parametrize("batch_moments", [0, 1])
def test_running_sums_equal_the_samples_added_in_call_order(pkg, O, batch_moments):
    shape = (40, 12, 17)
    with _perturbed_run(pkg, O, shape, 0) as a, _perturbed_run(pkg, O, shape, 0) as b:
        zeros, n = a.stats_get()  # before anything was accumulated
        assert n == 0 and zeros.shape == (24, 17) and not zeros.any()
        a.tune("batch_moments", batch_moments)
        a.stats_reset()
        bytes_before = a.device_bytes()  # nothing is allocated before the first pass
        want = np.zeros((24, 17))
        for _ in range(5):
            a.step(2)
            a.stats_accumulate()
            b.step(2)
            want = want + b.plane_sums()
        got, n = a.stats_get()
        assert n == 5 and np.array_equal(got, want)
        fa, fb = a.fields(), b.fields()
        for name in pkg.FIELDS:  # sampling does not disturb the run
            assert np.array_equal(fa[name], fb[name]), name
        a.stats_reset()
        got, n = a.stats_get()
        assert n == 0 and not got.any()
        held = a.device_bytes()
        assert held > bytes_before  # partial sums, results and running sums are counted ...
        a.stats_accumulate()
        got, n = a.stats_get()
        assert n == 1 and np.array_equal(got, b.plane_sums())
        assert a.device_bytes() == held  # ... and allocated once


def test_running_sums_of_a_group(pkg, O):
    po = O.default_params(40, 12, 17)
    po.pb_iterations = 20
    p = _mirror(pkg, po)
    with pkg.Group(p, 2, devices=[0, 0]) as a, pkg.Group(p, 2, devices=[0, 0]) as b:
        for g in (a, b):
            g.initialization()
            g.set_fields(O.perturb_fields(po, g.fields()))
            g.fast_Poisson()
            g.init_equilibrium()
        zeros, n = a.stats_get()
        assert n == 0 and zeros.shape == (24, 17) and not zeros.any()
        a.stats_reset()
        want = np.zeros((24, 17))
        for _ in range(5):
            a.step(2)
            a.stats_accumulate()
            b.step(2)
            want = want + b.plane_sums()
        got, n = a.stats_get()
        assert n == 5 and np.array_equal(got, want)
        fa, fb = a.fields(), b.fields()
        for name in pkg.FIELDS:
            assert np.array_equal(fa[name], fb[name]), name
        a.stats_reset()
        got, n = a.stats_get()
        assert n == 0 and not got.any()


# ---- 5. after a lazy solve ------------------------------------------------------------------------------

def test_plane_sums_right_after_a_lazy_solve(pkg, O):
    shape = (40, 12, 17)
    with _perturbed_run(pkg, O, shape, 0) as lazy, _perturbed_run(pkg, O, shape, 0, lazy_efield=0) as eager:
        lazy.step(7)   # nothing has looked at phi or E since
        eager.step(7)
        a, b = lazy.plane_sums(), eager.plane_sums()
        assert np.array_equal(a, b)
        assert np.abs(a[pkg.PROFILE_ID["Ez"]]).max() > 0.0 and np.abs(a[pkg.PROFILE_ID["q_Ez"]]).max() > 0.0


# ---- 6. files ---------------------------------------------------------------------------------------------

def _read_profiles(path):
    lines = open(path).read().splitlines()
    h = lines[0].split(" ")
    assert h[:3] == ["#", "ekpnp", "profiles"] and h[3::2] == ["nx", "ny", "nz", "z0", "nz_local", "samples", "time"], lines[0]
    hdr = dict(zip(h[3::2], h[4::2]))
    names = lines[1].split(" ")
    assert names[:3] == ["#", "z", "zcoord"]
    rows = [ln.split(" ") for ln in lines[2:]]
    assert all(len(r) == 2 + 24 for r in rows)
    z = [int(r[0]) for r in rows]
    data = np.array([[float(v) for v in r[1:]] for r in rows])
    return hdr, names[3:], z, data[:, 0], data[:, 1:].T  # means as [24][rows]


def test_save_profiles_round_trips(pkg, O, tmp_path):
    shape = (40, 12, 17)
    nodes = shape[0] * shape[1]
    with _perturbed_run(pkg, O, shape, 3) as s:
        # no sample yet: the instantaneous means of the current fields
        s.save_profiles(str(tmp_path / "now.dat"), 0.25)
        hdr, names, z, zc, means = _read_profiles(tmp_path / "now.dat")
        assert (hdr["samples"], float(hdr["time"])) == ("0", 0.25)
        assert np.array_equal(means, s.plane_sums() / float(nodes))
        for _ in range(3):
            s.step(1)
            s.stats_accumulate()
        acc, n = s.stats_get()
        s.save_profiles(str(tmp_path / "ctx.dat"), s.t)
        hdr, names, z, zc, means = _read_profiles(tmp_path / "ctx.dat")
        assert [int(hdr[k]) for k in ("nx", "ny", "nz", "z0", "nz_local", "samples")] == [40, 12, 17, 0, 17, 3] and n == 3
        assert float(hdr["time"]) == s.t
        assert names == pkg.PROFILE_NAMES and z == list(range(17))
        assert np.array_equal(zc, np.arange(17) * s.p.dz)
        assert np.array_equal(means, acc / float(n * nodes))
    po = O.default_params(*shape)
    po.pb_iterations = 20
    p = _mirror(pkg, po)
    with pkg.Group(p, 2, devices=[0, 0]) as g:
        g.initialization()
        g.set_fields(O.perturb_fields(po, g.fields()))
        g.fast_Poisson()
        g.init_equilibrium()
        for _ in range(2):
            g.step(2)
            g.stats_accumulate()
        acc, n = g.stats_get()
        g.save_profiles(str(tmp_path / "grp.dat"), g.t)
        hdr, names, z, zc, means = _read_profiles(tmp_path / "grp.dat")
        assert [int(hdr[k]) for k in ("nx", "ny", "nz", "z0", "nz_local", "samples")] == [40, 12, 17, 0, 17, 2] and n == 2
        assert float(hdr["time"]) == g.t and names == pkg.PROFILE_NAMES and z == list(range(17))
        assert np.array_equal(means, acc / float(n * nodes))
    with pkg.Solver(p, rank=1, nranks=2, slab=True) as s:  # a slab on its own writes its own planes
        s.set_fields(_random_fields(pkg, s.shape, 3))
        s.save_profiles(str(tmp_path / "slab.dat"), 0.0)
        hdr, names, z, zc, means = _read_profiles(tmp_path / "slab.dat")
        assert (int(hdr["z0"]), int(hdr["nz_local"])) == (s.z0, s.nz_local) == (8, 9) and z == list(range(8, 17))
        assert np.array_equal(means, s.plane_sums() / float(nodes))
        with pytest.raises(pkg.EkpnpError):
            s.save_profiles(str(tmp_path / "no_such_directory" / "x.dat"), 0.0)


# ---- 7. the driver ----------------------------------------------------------------------------------------

def _run_driver(args, out):
    out.mkdir()
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (args, r.stderr[-2000:])
    return out


@pytest.mark.parametrize("extra", [[], ["--devices", "0,0,0"]])
def test_driver_accumulates_every_n_iterations(pkg, tmp_path, extra):
    assert os.path.exists(EXE), "ekpnp_main not built"
    geo = ["--nx", "40", "--ny", "6", "--nz", "33", "--steps", "47", "--nsave", "15", "--print-current", "10", "--uw", "3e-4"]
    plain = _run_driver([*geo, *extra], tmp_path / "plain")
    loop = _run_driver([*geo, *extra, "--profiles-every", "4"], tmp_path / "loop")
    batch = _run_driver([*geo, *extra, "--profiles-every", "4", "--batch", "1"], tmp_path / "batch")
    assert not (plain / "profiles.dat").exists()
    hdr, names, z, zc, means = _read_profiles(loop / "profiles.dat")
    assert hdr["samples"] == "11" and z == list(range(33)) and names == pkg.PROFILE_NAMES
    assert (int(hdr["z0"]), int(hdr["nz_local"]), int(hdr["nz"])) == (0, 33, 33)
    assert np.isfinite(means).all() and means[pkg.PROFILE_ID["rho"]].min() > 0.0
    assert (loop / "profiles.dat").read_bytes() == (batch / "profiles.dat").read_bytes()
    for f in ("data.dat", "umax.dat", "data_end.dat"):
        a = (plain / f).read_bytes()
        assert len(a) > 0 and a == (loop / f).read_bytes() and a == (batch / f).read_bytes(), f


def test_driver_profiles_of_one_context_and_of_four_slabs(pkg, tmp_path):
    """The one sample is the final state (--profiles-every 40 of 40 steps), the state whose rho, c, cn, phi, T
    tests/test_group_gpu.py holds pointwise to 1e-9 * max|field| between the two runs; a plane mean cannot differ by more than
    the largest pointwise difference.  (Velocity and flux columns are rounding noise around zero in this x-y-uniform start.)"""
    assert os.path.exists(EXE), "ekpnp_main not built"
    geo = ["--nx", "24", "--ny", "6", "--nz", "32", "--steps", "40", "--nsave", "15", "--print-current", "10", "--profiles-every", "40"]
    one = _run_driver(geo, tmp_path / "one")
    four = _run_driver([*geo, "--devices", "0,0,0,0"], tmp_path / "four")
    h1, _, z1, _, m1 = _read_profiles(one / "profiles.dat")
    h4, _, z4, _, m4 = _read_profiles(four / "profiles.dat")
    assert h1 == h4 and h1["samples"] == "1" and z1 == z4 == list(range(32))
    for q in (0, 1, 2, 3, 10):
        a, b = m1[q], m4[q]
        assert np.abs(a).max() > 0.0
        assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max(), (pkg.PROFILE_NAMES[q], np.abs(a - b).max(), np.abs(a).max())
