"""GPU tests of the histograms, joint histograms, value ranges and the histogram time series (csrc/hist.hip; include/ekpnp.h:
ekpnp_hist_planes, ekpnp_value_range, ekpnp_hist_* and the ekpnp_group_* spellings; `ekpnp_main --hist-every N`).

A count is an integer, so every comparison here is exact (np.array_equal on int64): against a numpy transcription of the index
function of include/ekpnp.h (tests/test_hist_cpu.py holds the library's host function against the same transcription), across
buffer modes and decompositions, and of the ring against a twin's synchronous counts.  Shapes: R, W, V of tests/test_modes_gpu.py;
B, whose plane of 9 100 nodes takes two workgroups; O, whose plane of 1 155 nodes is odd, so that its odd planes start at an odd
double and take the kernel's 8-byte path."""
import os
import subprocess

import numpy as np
import pytest

from _observer_pairs import ring_spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
R = (40, 12, 17)
W = (70, 66, 13)
V = (128, 36, 9)
B = (130, 70, 4)
O = (35, 33, 5)
SHAPES = {"R": R, "W": W, "V": V, "B": B, "O": O}

# ranges chosen inside what _random_fields spreads (uz, ux: 1e-3; c, cn: 30, so q within 60; T: 1; phi: 5e-3): both outer cells fill
UZ = ("uz", 16, -0.5e-3, 0.7e-3)
SPECS = {
    "uz": (UZ, None),
    "q129": (("q", 129, -25.0, 31.5), None),
    "uz_T": (("uz", 7, -0.5e-3, 0.7e-3), ("T", 5, -0.6, 0.8)),
    "q_uz": (("q", 64, -25.0, 31.5), ("uz", 64, -0.9e-3, 0.8e-3)),
    "uz_q": (("uz", 3, -0.5e-3, 0.7e-3), ("q", 4, -25.0, 31.5)),
    "q_q": (("q", 5, -25.0, 31.5), ("q", 3, -40.0, 10.0)),
    "phi4096": (("phi", 4096, -3e-3, 4e-3), None),
    "T_1x4096": (("T", 1, -0.6, 0.8), ("ux", 4096, -0.9e-3, 0.8e-3)),  # the largest cell count a spec can have: 3 * 4098
}


def _params(pkg, shape, in_place=0):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    p.in_place = in_place
    return p


def _random_fields(pkg, shape_zyx, seed):
    rng = np.random.default_rng(seed)
    scale = {"rho": 1000.0, "c": 30.0, "cn": 30.0, "phi": 5e-3, "T": 1.0, "Ex": 1e5, "Ey": 1e5, "Ez": 1e5}
    return {n: scale.get(n, 1e-3) * rng.uniform(-1.0, 1.0, size=shape_zyx) for n in pkg.FIELDS}


def _value(f, name):
    return f["c"] - f["cn"] if name == "q" else f[name]  # one FP64 subtraction per node


def _index(axis, v):
    """the index function of include/ekpnp.h in numpy float64, every operation rounded once"""
    _, n, lo, hi = axis
    lo, hi = np.float64(lo), np.float64(hi)
    scale = np.float64(n) / (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (v - lo) * scale
        inside = ~(v != v) & ~(v < lo) & ~(v >= hi)
        k = np.minimum(np.where(inside, s, 0.0).astype(np.int64), n - 1)
    return np.where(v != v, -1, np.where(v < lo, 0, np.where(v >= hi, n + 1, 1 + k)))


def _counts(f, a, b=None):
    """(counts[nz, a.n + 2(, b.n + 2)], nonfinite[nz]) of the fields f by the definition"""
    ia = _index(a, _value(f, a[0]))
    nz = ia.shape[0]
    if b is None:
        shape, cell, bad = (a[1] + 2,), ia, ia < 0
    else:
        ib = _index(b, _value(f, b[0]))
        shape, cell, bad = (a[1] + 2, b[1] + 2), ia * (b[1] + 2) + ib, (ia < 0) | (ib < 0)
    ncell = int(np.prod(shape))
    counts = np.stack([np.bincount(cell[z][~bad[z]].ravel(), minlength=ncell).reshape(shape) for z in range(nz)]).astype(np.int64)
    return counts, bad.reshape(nz, -1).sum(axis=1).astype(np.int64)


def _equal(got, want):
    return all(g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def fields(pkg):
    """random fields of every shape (made once, never modified)"""
    return {k: _random_fields(pkg, (s[2], s[1], s[0]), 31) for k, s in SHAPES.items()}


@pytest.fixture(scope="module")
def reference(pkg, fields):
    """the definition's counts of W's random fields for every spec (computed once, never modified)"""
    return {k: _counts(fields["W"], a, b) for k, (a, b) in SPECS.items()}


# ---- 1. counts against numpy ---------------------------------------------------------------------------------

def test_counts_of_every_spec_equal_the_definition(pkg, fields, reference):
    nx, ny, nz = W
    with pkg.Solver(_params(pkg, W)) as s:
        s.set_fields(fields["W"])
        for k, (a, b) in SPECS.items():
            counts, nonfinite = s.hist_planes(a, b)
            want = reference[k]
            assert _equal((counts, nonfinite), want), k
            flat = counts.reshape(nz, -1)
            assert (flat.sum(axis=1) + nonfinite == nx * ny).all(), k
            if b is None:
                assert (counts[:, 0] > 0).all() and (counts[:, -1] > 0).all(), k  # under- and overflow cells are both filled
            else:
                assert counts[:, 0, :].sum() > 0 and counts[:, -1, :].sum() > 0 and counts[:, :, 0].sum() > 0 and counts[:, :, -1].sum() > 0, k


@pytest.mark.parametrize("shape", ["R", "V", "B", "O"])
def test_counts_on_the_other_shapes(pkg, fields, shape):
    nx, ny, nz = SHAPES[shape]
    f = fields[shape]
    with pkg.Solver(_params(pkg, SHAPES[shape])) as s:
        s.set_fields(f)
        for k in ("uz", "q129", "uz_T", "q_uz", "q_q"):
            a, b = SPECS[k]
            counts, nonfinite = s.hist_planes(a, b)
            assert _equal((counts, nonfinite), _counts(f, a, b)), (shape, k)
            assert (counts.reshape(nz, -1).sum(axis=1) + nonfinite == nx * ny).all(), (shape, k)


# ---- 2. edge values --------------------------------------------------------------------------------------------

def _edge_values(lo, hi, n):
    lo, hi = np.float64(lo), np.float64(hi)
    edges = lo + np.arange(n + 1, dtype=np.float64) * (hi - lo) / n
    return np.concatenate([[lo, hi, np.nextafter(hi, lo), np.nextafter(lo, -np.inf), -0.0, 0.0, np.inf, -np.inf, np.nan], edges,
                           np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])


@pytest.mark.parametrize("n", [1, 2, 7, 4096])
def test_edge_values_land_where_the_host_function_says(pkg, n):
    nx, ny, nz = B
    lo, hi = -3.7e-4, 9.1e-4
    ev = _edge_values(lo, hi, n)
    assert len(ev) <= 2 * nx * ny
    vals = np.resize(ev, (2, ny * nx))                   # the edge values, again and again, over planes 1 and 2
    other = np.resize(np.array([0.1, np.nan, np.inf, -np.inf, 0.5, -0.25, 0.75]), (2, ny * nx))  # period 7: every pairing occurs
    uz = np.zeros((nz, ny, nx))
    T = np.zeros((nz, ny, nx))
    uz[1:3], T[1:3] = vals.reshape(2, ny, nx), other.reshape(2, ny, nx)
    uz[3] = vals[0, ::-1].reshape(ny, nx)
    a, b = ("uz", n, lo, hi), ("T", 1, 0.0, 0.5)
    ia = pkg.hist_bin(lo, hi, n, vals)                  # the host function
    ib = pkg.hist_bin(0.0, 0.5, 1, other)
    with pkg.Solver(_params(pkg, B)) as s:
        s.set_field("uz", uz)
        s.set_field("T", T)
        c1, nf1 = s.hist_planes(a)
        c2, nf2 = s.hist_planes(a, b)
    bad = (ia < 0) | (ib < 0)
    total1 = np.zeros(n + 2, dtype=np.int64)
    for z in (0, 1):
        nan1 = int((ia[z] < 0).sum())
        assert nan1 == np.isnan(vals[z]).sum() > 0
        want1 = np.bincount(ia[z][ia[z] >= 0], minlength=n + 2)
        total1 += want1
        assert np.array_equal(c1[1 + z], want1) and nf1[1 + z] == nan1, z
        if z == 0:
            assert np.array_equal(c1[3], want1) and nf1[3] == nan1    # the same values in another order
        want2 = np.bincount((ia[z] * 3 + ib[z])[~bad[z]], minlength=(n + 2) * 3).reshape(n + 2, 3)
        assert np.array_equal(c2[1 + z], want2) and nf2[1 + z] == bad[z].sum(), z
        assert bad[z].sum() > nan1 > 0                                # a NaN in one value of the pair only
        assert want2[:, 0].sum() > 0 and want2[:, 2].sum() > 0        # -Inf and +Inf of the second value
    assert c1[0, pkg.hist_bin(lo, hi, n, 0.0)] == nx * ny and nf1[0] == 0
    assert (total1 > 0).all()                                         # every cell, under- and overflow included, is hit


# ---- 3. a constant field: all 64 lanes of a wavefront at one counter -------------------------------------

def test_a_constant_field_fills_one_cell(pkg):
    nx, ny, nz = W
    with pkg.Solver(_params(pkg, W)) as s:
        s.set_field("uz", np.full(s.shape, 0.25e-3))
        s.set_field("c", np.full(s.shape, 12.0))
        s.set_field("cn", np.full(s.shape, 7.5))
        counts, nonfinite = s.hist_planes(UZ)
        k = pkg.hist_bin(UZ[2], UZ[3], UZ[1], 0.25e-3)
        want = np.zeros((nz, UZ[1] + 2), dtype=np.int64)
        want[:, k] = nx * ny
        assert 1 <= k <= UZ[1] and _equal((counts, nonfinite), (want, np.zeros(nz, dtype=np.int64)))
        a, b = SPECS["q_uz"]
        counts, nonfinite = s.hist_planes(a, b)
        want = np.zeros((nz, 66, 66), dtype=np.int64)
        want[:, pkg.hist_bin(a[2], a[3], a[1], 4.5), pkg.hist_bin(b[2], b[3], b[1], 0.25e-3)] = nx * ny
        assert _equal((counts, nonfinite), (want, np.zeros(nz, dtype=np.int64)))
        v = np.full(s.shape, 0.25e-3)
        v[3] = np.nan                                   # a plane of NaNs: the same, at the nonfinite counter
        v[5, 7, 11] = 0.5e-3                            # one lane of one wavefront elsewhere
        s.set_field("uz", v)
        counts, nonfinite = s.hist_planes(UZ)
        assert counts[3].sum() == 0 and nonfinite[3] == nx * ny and nonfinite.sum() == nx * ny
        k2 = pkg.hist_bin(UZ[2], UZ[3], UZ[1], 0.5e-3)
        assert k2 != k and counts[5, k2] == 1 and counts[5, k] == nx * ny - 1 and counts[5].sum() == nx * ny


# ---- 4. the same counts however the lattice is held ---------------------------------------------------------

HELD = ("uz", "q129", "uz_T", "q_uz")


def test_in_place_slabs_groups_and_a_bound_array_give_the_same_counts(pkg, fields, reference):
    import torch

    f = fields["W"]
    p = _params(pkg, W)
    with pkg.Solver(_params(pkg, W, in_place=1)) as s:
        s.set_fields(f)
        for k in HELD:
            assert _equal(s.hist_planes(*SPECS[k]), reference[k]), ("in place", k)
    for rank in range(3):
        with pkg.Solver(p, rank=rank, nranks=3, slab=True) as s:
            z0, nzl = s.z0, s.nz_local
            s.set_fields({n: v[z0:z0 + nzl] for n, v in f.items()})
            for k in HELD:
                assert _equal(s.hist_planes(*SPECS[k]), [w[z0:z0 + nzl] for w in reference[k]]), ("slab", rank, k)
    for nslabs in (2, 3):
        with pkg.Group(p, nslabs, devices=[0] * nslabs) as g:
            g.set_fields(f)
            for k in HELD:
                assert _equal(g.hist_planes(*SPECS[k]), reference[k]), ("group", nslabs, k)
    with pkg.Solver(p) as s:  # uz at an address that is 8 mod 16: the 8-byte loads
        n = int(np.prod(s.shape))
        pool = torch.zeros(n + 3, dtype=torch.float64, device="cuda")
        view = pool[1:1 + n] if pool.data_ptr() % 16 == 0 else pool[2:2 + n]
        assert view.data_ptr() % 16 == 8
        s.bind_field("uz", view.data_ptr())
        s.set_fields(f)
        for k in HELD:
            assert _equal(s.hist_planes(*SPECS[k]), reference[k]), ("bound", k)
        assert float(pool[0]) == 0.0 and float(pool[-1]) == 0.0


def test_the_marginals_of_a_joint_histogram_are_the_1d_histograms(pkg, fields, reference):
    joint, nonfinite = reference["uz_T"]
    a, b = SPECS["uz_T"]
    assert nonfinite.sum() == 0
    with pkg.Solver(_params(pkg, W)) as s:
        s.set_fields(fields["W"])
        got, _ = s.hist_planes(a, b)
        assert np.array_equal(got.sum(axis=2), s.hist_planes(a)[0])
        assert np.array_equal(got.sum(axis=1), s.hist_planes(b)[0])
    assert np.array_equal(got, joint)


# ---- 5. value_range -------------------------------------------------------------------------------------------

def test_value_range_is_nanmin_and_nanmax_per_plane(pkg, fields):
    nx, ny, nz = W
    f = {n: v.copy() for n, v in fields["W"].items()}
    rng = np.random.default_rng(5)
    for name in ("uz", "c", "T"):
        f[name].reshape(-1)[rng.integers(0, f[name].size, size=200)] = np.nan
    f["T"][4] = np.nan                  # a plane of NaNs only
    f["uz"][2, 3, 4] = np.inf
    f["uz"][6, 0, 0] = -np.inf
    p = _params(pkg, W)
    with pkg.Solver(p) as s, pkg.Group(p, 3, devices=[0, 0, 0]) as g:
        s.set_fields(f)
        g.set_fields(f)
        for name in ("uz", "q", "T", "phi", "rho"):
            v = _value(f, name).reshape(nz, -1)
            lo, hi = s.value_range(name)
            for z in range(nz):
                if np.isnan(v[z]).all():
                    assert (lo[z], hi[z]) == (np.inf, -np.inf), (name, z)
                else:
                    assert lo[z] == np.nanmin(v[z]) and hi[z] == np.nanmax(v[z]), (name, z, lo[z], hi[z])
            glo, ghi = g.value_range(name)
            assert np.array_equal(glo, lo) and np.array_equal(ghi, hi), name
        assert s.value_range("T")[0][4] == np.inf and s.value_range("uz")[1][2] == np.inf and s.value_range("uz")[0][6] == -np.inf
        with pytest.raises(pkg.EkpnpError):
            s.value_range(12)


# ---- 6. the ring ------------------------------------------------------------------------------------------------

SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)


def _seeded_start(pkg, s, **knobs):
    for k, v in knobs.items():
        s.tune(k, v)
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


_ring_spec = ring_spec   # axes from the start fields' own ranges (tests/_observer_pairs.py, shared with the pair tests; second axis phi)


@pytest.mark.parametrize("stride, batch, joint, planes", [(1, 0, False, (1, 15)), (3, 0, True, (1, 15)), (1, 1, True, (8, 8)), (3, 1, False, (0, 16))])
def test_ring_rows_equal_a_twins_synchronous_counts(pkg, stride, batch, joint, planes):
    nx, ny, nz = R
    z_lo, z_hi = planes
    with pkg.Solver(_params(pkg, R)) as a, pkg.Solver(_params(pkg, R)) as b:
        _seeded_start(pkg, a, batch_moments=batch)
        _seeded_start(pkg, b)
        assert a.hist_count() == (0, 0)
        spec = pkg.hist_spec(*_ring_spec(b, z_lo, z_hi, joint))
        a.hist_arm(spec, planes=planes, capacity=4)
        want = []
        for k in range(1, 7):
            a.step(stride)
            a.hist_record(k * stride, a.t)
            b.step(stride)
            c, nf = b.hist_planes(spec)
            want.append((k * stride, b.t, c[z_lo:z_hi + 1].sum(axis=0), nf[z_lo:z_hi + 1].sum()))
        assert a.hist_count() == (6, 2)  # the ring held four: the two oldest rows are gone
        steps, times, counts, nonfinite = a.hist_read()
        assert counts.shape == (4,) + spec.cell_shape and counts.dtype == np.int64 and nonfinite.shape == (4,)
        assert steps.tolist() == [w[0] for w in want[2:]] and times.tolist() == [w[1] for w in want[2:]]
        for row, nf, w in zip(counts, nonfinite, want[2:]):
            assert np.array_equal(row, w[2]) and nf == w[3], (w[0], row, w[2])
            assert row.sum() + nf == nx * ny * (z_hi - z_lo + 1)
        assert (counts[-1] != counts[0]).any()  # the distribution moves
        # read: oldest first, range checked
        s1, _, c1, _ = a.hist_read(1, 2)
        assert s1.tolist() == steps[1:3].tolist() and np.array_equal(c1, counts[1:3])
        with pytest.raises(pkg.EkpnpError):
            a.hist_read(2, 3)
        # disarmed: the rows stay readable, record is refused; armed again: an empty ring
        a.hist_disarm()
        assert np.array_equal(a.hist_read()[2], counts)
        with pytest.raises(pkg.EkpnpError):
            a.hist_record(7, 0.0)
        a.hist_arm(UZ, planes=(2, 3), capacity=3)
        assert a.hist_count() == (0, 0) and a.hist_read()[2].shape == (0, UZ[1] + 2)


@pytest.mark.parametrize("nslabs, planes", [(2, (1, 15)), (3, (6, 6))])
def test_ring_on_a_group_equals_the_single_context(pkg, nslabs, planes):
    """the group steps; after every step a single context is handed the group's c, cn and phi and counted synchronously"""
    z_lo, z_hi = planes
    p = _params(pkg, R)
    with pkg.Group(p, nslabs, devices=[0] * nslabs) as g, pkg.Solver(p) as s:
        _seeded_start(pkg, g)
        for n in ("c", "cn", "phi"):
            s.set_field(n, g.get_field(n))
        spec = pkg.hist_spec(*_ring_spec(s, z_lo, z_hi, True))
        g.hist_arm(spec, planes=planes, capacity=8)
        want = []
        for k in range(1, 4):
            g.step(1)
            g.hist_record(k, g.t)
            for n in ("c", "cn", "phi"):
                s.set_field(n, g.get_field(n))
            c, nf = s.hist_planes(spec)
            want.append((c[z_lo:z_hi + 1].sum(axis=0), nf[z_lo:z_hi + 1].sum()))
        assert g.hist_count() == (3, 0)
        steps, _, counts, nonfinite = g.hist_read()
        assert steps.tolist() == [1, 2, 3]
        for row, nf, w in zip(counts, nonfinite, want):
            assert np.array_equal(row, w[0]) and nf == w[1]
            assert row.sum() + nf == R[0] * R[1] * (z_hi - z_lo + 1)


def test_a_slab_without_a_plane_of_the_range_records_zeros(pkg, fields):
    f = fields["W"]
    p = _params(pkg, W)
    for rank, planes, expect_zero in ((2, (1, 2), True), (0, (1, 2), False), (0, (12, 12), True), (1, (3, 11), False)):
        with pkg.Solver(p, rank=rank, nranks=3, slab=True) as s:
            z0, nzl = s.z0, s.nz_local
            s.set_fields({n: v[z0:z0 + nzl] for n, v in f.items()})
            s.hist_arm(UZ, planes=planes, capacity=2)
            s.hist_record(1, 0.0)
            _, _, counts, nonfinite = s.hist_read()
            lo, hi = max(planes[0], z0), min(planes[1], z0 + nzl - 1)
            want = _counts({"uz": f["uz"][lo:hi + 1]}, UZ)[0].sum(axis=0) if hi >= lo else np.zeros(UZ[1] + 2, dtype=np.int64)
            assert (hi < lo) == expect_zero, (rank, planes, z0, nzl)
            assert np.array_equal(counts[0], want) and nonfinite[0] == 0 and (counts[0].sum() == 0) == expect_zero, (rank, planes)


# ---- 7. the run is left alone -----------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_recording_leaves_the_step_graph_and_the_run_alone(pkg):
    with pkg.Solver(_params(pkg, R)) as a, pkg.Solver(_params(pkg, R)) as b:
        _seeded_start(pkg, a)
        _seeded_start(pkg, b)
        a.step(5)
        b.step(5)
        state = a.graph_state()
        assert state == 1
        bytes_before = a.device_bytes()
        a.hist_arm(("q", 32, -1.0, 1.0), ("phi", 8, 0.0, 1.0), planes=(1, 15), capacity=8)
        assert a.graph_state() == state and a.device_bytes() > bytes_before
        for k in range(6):
            a.step(1)
            a.hist_record(6 + k, a.t)
        b.step(6)
        assert a.graph_state() == state and b.graph_state() == state and a.hist_count() == (6, 0)
        fa, fb = a.fields(), b.fields()
        for n in pkg.FIELDS:
            assert np.array_equal(_bits(fa[n]), _bits(fb[n])), n
        assert b.device_bytes() == bytes_before  # a context that never calls the new entry points allocates nothing new


# ---- 8. the driver ----------------------------------------------------------------------------------------------

def _run_driver(args, out, code=0):
    out.mkdir()
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1", EKPNP_PLACEMENT_TRIES="1")  # the child shares device 0 with this process
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == code, (args, r.stderr[-2000:])
    return out, r.stderr


def _read_hist(path):
    lines = open(path).read().splitlines()
    w = lines[0].split()
    assert w[:3] == ["#", "ekpnp", "hist"] and w[3:9:2] == ["nx", "ny", "nz"] and w[9] == "a"
    hdr = dict(nx=int(w[4]), ny=int(w[6]), nz=int(w[8]), a=(w[10], int(w[11]), float(w[12]), float(w[13])), b=None)
    k = 14
    if w[k] == "b":
        hdr["b"] = (w[k + 1], int(w[k + 2]), float(w[k + 3]), float(w[k + 4]))
        k += 5
    assert w[k:k + 8:2] == ["z_lo", "z_hi", "recorded", "dropped"] and len(w) == k + 8
    hdr.update(z_lo=int(w[k + 1]), z_hi=int(w[k + 3]), recorded=int(w[k + 5]), dropped=int(w[k + 7]))
    rows = [ln.split() for ln in lines[1:]]
    assert all(" ".join(r) == ln for r, ln in zip(rows, lines[1:]))  # single spaces
    return hdr, [int(r[0]) for r in rows], [float(r[1]) for r in rows], np.array([[int(x) for x in r[2:]] for r in rows], dtype=np.int64)


GEO = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "6", "--seed-pattern", "squares", "--seed-modes", "1,1"]


def test_driver_writes_the_rows_of_the_library_calls(pkg, tmp_path):
    assert os.path.exists(EXE), "ekpnp_main not built"
    p = pkg.default_params(40, 12, 17)
    want = []
    with pkg.Solver(p) as s:  # the driver's loop, call by call
        s.initialization()
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-3, noise=0.0, relative=True, seed=1))
        s.fast_Poisson()
        s.init_equilibrium()
        a, b = _ring_spec(s, 1, 15, True)
        b = ("phi", 64, b[2], b[3])  # (--hist-bins2 is left at its default)
        t = 0.0
        for i in range(6):
            s.stream_collide_save(t)
            s.fast_Poisson()
            t = t + p.dt
            if (i + 1) % 2 == 0:
                c, nf = s.hist_planes(a, b)
                want.append((i + 1, t, np.concatenate([[nf[1:16].sum()], c[1:16].sum(axis=0).ravel()])))
    flags = ["--hist-every", "2", "--hist-value", "q", "--hist-bins", str(a[1]), "--hist-range", f"{a[2]!r},{a[3]!r}",
             "--hist-value2", "phi", "--hist-range2", f"{b[2]!r},{b[3]!r}"]
    plain, _ = _run_driver(GEO, tmp_path / "plain")
    again, _ = _run_driver(GEO, tmp_path / "again")
    loop, _ = _run_driver([*GEO, *flags], tmp_path / "loop")
    batch, _ = _run_driver([*GEO, *flags, "--batch", "1"], tmp_path / "batch")
    hdr, steps, times, rows = _read_hist(loop / "hist.dat")
    assert hdr == dict(nx=40, ny=12, nz=17, a=a, b=b, z_lo=1, z_hi=15, recorded=3, dropped=0)
    assert steps == [w[0] for w in want] and times == [w[1] for w in want]
    assert rows.shape == (3, 1 + 26 * 66)
    for row, w in zip(rows, want):
        assert np.array_equal(row, w[2]), w[0]
        assert row.sum() == 40 * 12 * 15
    assert (rows[-1] != rows[0]).any() and (rows[:, 1:] > 0).sum() > 20  # a distribution, and one that moves
    assert (loop / "hist.dat").read_bytes() == (batch / "hist.dat").read_bytes()
    assert not (plain / "hist.dat").exists()
    for f in ("data.dat", "umax.dat", "data_end.dat"):
        x = (plain / f).read_bytes()
        assert len(x) > 0 and x == (again / f).read_bytes() and x == (loop / f).read_bytes() and x == (batch / f).read_bytes(), f
    assert sorted(os.listdir(plain)) == sorted(os.listdir(again)) and sorted(os.listdir(loop)) == sorted(os.listdir(plain) + ["hist.dat"])
    # one plane, one axis; and a bad flag exits 2 with the library's message
    one, _ = _run_driver([*GEO, "--hist-every", "3", "--hist-value", "uz", "--hist-bins", "5", "--hist-range", "-1e-9,1e-9", "--hist-planes", "8,8"],
                         tmp_path / "one")
    hdr, steps, _, rows = _read_hist(one / "hist.dat")
    assert hdr["a"] == ("uz", 5, -1e-9, 1e-9) and hdr["b"] is None and (hdr["z_lo"], hdr["z_hi"]) == (8, 8) and steps == [3, 6]
    assert rows.shape == (2, 8) and (rows.sum(axis=1) == 480).all()
    for bad, number in ((["--hist-range", "2,1"], "hi = 1 "), (["--hist-range", "0,1", "--hist-planes", "3,17"], "17"),
                        (["--hist-range", "0,1", "--hist-bins", "5000"], "5000"), (["--hist-range", "0,1", "--hist-value", "w"], "w")):
        _, err = _run_driver([*GEO, "--hist-every", "2", *bad], tmp_path / ("bad" + number.strip().replace(" ", "_").replace("=", "")), code=2)
        assert number in err, err
