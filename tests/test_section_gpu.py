"""GPU tests of the sections and their time series (csrc/section.hip; include/ekpnp.h: ekpnp_section, ekpnp_section_save,
ekpnp_section_* and the ekpnp_group_* spellings; `ekpnp_main --section-every N / --section-full-every N`).

Every map entry is ekpnp_section_sum of its line, so every comparison but one is on the float64 BIT PATTERN: against a numpy loop of
the definition (tests/test_section_cpu.py holds the library's host function against the same loop), across buffer modes and
decompositions, and of the ring against a twin's synchronous sections.  The one toleranced check holds a section against
ekpnp_plane_sums, with the a-priori bound of tests/test_profiles_gpu.py.  Shapes: those of tests/test_hist_gpu.py - R 40 x 12 x 17
is less than one run and one tile, W 70 x 66 x 13 one run plus a remainder on both axes, V 128 x 36 x 9 exactly two runs,
B 130 x 70 x 4 three runs and two tiles of rows, O 35 x 33 x 5 odd, so that its odd planes start at an odd double."""
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
R = (40, 12, 17)
W = (70, 66, 13)
V = (128, 36, 9)
B = (130, 70, 4)
O = (35, 33, 5)
SHAPES = {"R": R, "W": W, "V": V, "B": B, "O": O}
ACROSS = ("x", "y")
VALUE_SETS = {"all": None, "q": ["q"], "c_q": ["c", "q"], "phi_Ez": ["phi", "Ez"], "uz": ["uz"]}


def _params(pkg, shape, in_place=0):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    p.in_place = in_place
    return p


def _random_fields(pkg, shape_zyx, seed):
    rng = np.random.default_rng(seed)
    scale = {"rho": 1000.0, "c": 30.0, "cn": 30.0, "phi": 5e-3, "T": 1.0, "Ex": 1e5, "Ey": 1e5, "Ez": 1e5}
    return {n: scale.get(n, 1e-3) * rng.uniform(-1.0, 1.0, size=shape_zyx) for n in pkg.FIELDS}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(got, want):
    return got.shape == want.shape and got.dtype == np.float64 and np.array_equal(_bits(got), _bits(want))


def _value(f, name):
    return f["c"] - f["cn"] if name == "q" else f[name]  # one FP64 subtraction per node, before any addition


def _line_sums(v, across, lo, hi):
    """the definition as a numpy loop over [nz, ny, nx]: S = v[..., lo], then S = S + v[..., i], run by run"""
    t = v[:, :, lo:hi + 1] if across == "x" else np.moveaxis(v[:, lo:hi + 1, :], 1, 2)
    n = hi - lo + 1
    S = None
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, n, 64):
            r = t[..., i0].copy()
            for i in range(i0 + 1, min(i0 + 64, n)):
                r = r + t[..., i]
            S = r if S is None else S + r
    return S


def _names(pkg, values):
    return pkg.SECTION_VALUES if values is None else [n for n in pkg.SECTION_VALUES if n in values]


def _ranges(shape, across):
    n = shape[0] if across == "x" else shape[1]
    # unaligned: 65 terms from an odd start - 3 .. 67 along x; along y, where W has 66 rows, 1 .. 65
    return n, {"full": (0, n - 1), "first": (0, 0), "middle": (n // 2, n // 2), "last": (n - 1, n - 1), "unaligned": (3, 67) if across == "x" else (1, 65)}


@pytest.fixture(scope="module")
def fields(pkg):
    """random fields of every shape (made once, never modified)"""
    return {k: _random_fields(pkg, (s[2], s[1], s[0]), 47) for k, s in SHAPES.items()}


@pytest.fixture(scope="module")
def reference(pkg, fields):
    """reference(shape, name, across, lo, hi) -> [nz, nkeep] by the definition; every map is computed once and never modified"""
    cache = {}

    def get(shape, name, across, lo, hi):
        key = (shape, name, across, lo, hi)
        if key not in cache:
            cache[key] = _line_sums(_value(fields[shape], name), across, lo, hi)
            cache[key].setflags(write=False)
        return cache[key]

    return get


def _want(pkg, reference, shape, values, across, lo, hi, planes=None):
    rows = slice(None) if planes is None else list(planes)
    return np.stack([reference(shape, n, across, lo, hi)[rows] for n in _names(pkg, values)])


# ---- 1. W: every range, value set and plane choice ----------------------------------------------------------------

@pytest.mark.parametrize("across", ACROSS)
def test_sections_of_w_equal_the_definition(pkg, fields, reference, across):
    nx, ny, nz = W
    n, ranges = _ranges(W, across)
    assert ranges["unaligned"][1] - ranges["unaligned"][0] + 1 == 65 and ranges["unaligned"][1] < n
    with pkg.Solver(_params(pkg, W)) as s:
        s.set_fields(fields["W"])
        for rk, (lo, hi) in ranges.items():
            for vk, values in VALUE_SETS.items():
                for planes in (None, [0, 5, nz - 1]):
                    got = s.section(values, across, (lo, hi), planes)
                    want = _want(pkg, reference, "W", values, across, lo, hi, planes)
                    assert got.shape == (len(_names(pkg, values)), nz if planes is None else 3, ny if across == "x" else nx)
                    assert _same(got, want), (across, rk, vk, planes, np.argwhere(_bits(got) != _bits(want))[:5])
        assert _same(s.section(None, across), _want(pkg, reference, "W", None, across, 0, n - 1))  # range None: the whole axis
        lo, hi = ranges["middle"]
        f = fields["W"]
        cut = f["uz"][:, :, lo] if across == "x" else f["uz"][:, lo, :]
        assert _same(s.section(["uz"], across, (lo, hi))[0], cut)  # a cut is the field itself
        with pytest.raises(pkg.EkpnpError) as e:
            s.section(["uz"], across, (0, n))
        assert str(n) in str(e.value)


# ---- 2. the other shapes --------------------------------------------------------------------------------------------

UNALIGNED = {"R": {"x": (5, 37), "y": (1, 10)}, "V": {"x": (1, 127), "y": (2, 34)}, "B": {"x": (1, 129), "y": (3, 67)}, "O": {"x": (1, 33), "y": (2, 32)}}


@pytest.mark.parametrize("across", ACROSS)
@pytest.mark.parametrize("shape", ["R", "V", "B", "O"])
def test_sections_on_the_other_shapes(pkg, fields, reference, shape, across):
    nx, ny, nz = SHAPES[shape]
    n = nx if across == "x" else ny
    with pkg.Solver(_params(pkg, SHAPES[shape])) as s:
        s.set_fields(fields[shape])
        for lo, hi in ((0, n - 1), UNALIGNED[shape][across]):
            for values in (None, ["uz"], ["c", "q"]):
                got = s.section(values, across, (lo, hi))
                assert _same(got, _want(pkg, reference, shape, values, across, lo, hi)), (shape, across, lo, hi, values)
            got = s.section(["q", "uz"], across, (lo, hi), [0, nz - 1])
            assert _same(got, _want(pkg, reference, shape, ["q", "uz"], across, lo, hi, [0, nz - 1])), (shape, across, lo, hi)


# ---- 3. special values ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("across", ACROSS)
def test_special_values_stay_in_their_own_line(pkg, fields, across):
    nx, ny, nz = W
    f = {n: v.copy() for n, v in fields["W"].items()}
    planted = {(2, 7, 11): -0.0, (2, 40, 65): np.inf, (4, 65, 3): np.nan, (4, 0, 69): np.nan, (9, 33, 64): -np.inf}
    for (z, y, x), val in planted.items():
        f["uz"][z, y, x] = val
        f["c"][z, y, x] = val
    n = nx if across == "x" else ny
    with pkg.Solver(_params(pkg, W)) as s:
        s.set_fields(f)
        for (z, y, x), val in planted.items():  # a cut returns the planted bits
            at, keep = (x, y) if across == "x" else (y, x)
            got = s.section(["c", "uz"], across, (at, at), [z])   # (ascending id: c, then uz)
            assert _bits(got[0, 0, keep]) == _bits(val) and _bits(got[1, 0, keep]) == _bits(val), (z, y, x, val)
            cut = f["uz"][z, :, x] if across == "x" else f["uz"][z, y, :]
            assert _same(got[1, 0], cut)
        for lo, hi in ((0, n - 1), _ranges(W, across)[1]["unaligned"]):
            got = s.section(["c", "uz", "q"], across, (lo, hi))
            want = np.stack([_line_sums(_value(f, k), across, lo, hi) for k in ("c", "uz", "q")])
            assert np.array_equal(np.isnan(got), np.isnan(want))
            assert np.isnan(want).sum() >= 2 and np.isnan(want[0]).sum() <= 3   # the NaNs stay in their own lines
            ok = ~np.isnan(want)
            assert np.array_equal(_bits(got[ok]), _bits(want[ok]))   # every other entry is bit-equal
            assert np.isinf(got[0]).sum() >= 1


# ---- 4. the same bits however the lattice is held -----------------------------------------------------------------

HELD = [(None, "x", (0, 69)), (["c", "q"], "x", (3, 67)), (["uz", "phi"], "y", (0, 65)), (["q"], "y", (3, 65)), (["uz"], "x", (35, 35))]


def test_in_place_slabs_groups_and_a_bound_array_give_the_same_bits(pkg, fields, reference):
    import torch

    nx, ny, nz = W
    f = fields["W"]
    p = _params(pkg, W)
    chosen = [0, 5, nz - 1]
    with pkg.Solver(_params(pkg, W, in_place=1)) as s:
        s.set_fields(f)
        for values, across, (lo, hi) in HELD:
            assert _same(s.section(values, across, (lo, hi)), _want(pkg, reference, "W", values, across, lo, hi)), ("in place", values, across)
            assert _same(s.section(values, across, (lo, hi), chosen), _want(pkg, reference, "W", values, across, lo, hi, chosen))
    for rank in range(3):
        with pkg.Solver(p, rank=rank, nranks=3, slab=True) as s:
            z0, nzl = s.z0, s.nz_local
            s.set_fields({n: v[z0:z0 + nzl] for n, v in f.items()})
            for values, across, (lo, hi) in HELD:
                own = list(range(z0, z0 + nzl))
                assert _same(s.section(values, across, (lo, hi)), _want(pkg, reference, "W", values, across, lo, hi, own)), ("slab", rank)
                got = s.section(values, across, (lo, hi), chosen)
                want = _want(pkg, reference, "W", values, across, lo, hi, chosen).copy()
                for j, z in enumerate(chosen):
                    if not z0 <= z < z0 + nzl:
                        want[:, j, :] = 0.0  # a chosen plane the slab does not own: a row of +0.0
                assert _same(got, want), ("slab", rank, values, across)
            other = [z for z in (0, nz - 1) if not z0 <= z < z0 + nzl][:1]
            got = s.section(["uz", "q"], "x", (0, nx - 1), other)
            assert got.shape == (2, 1, ny) and not _bits(got).any()
    for nslabs in (2, 3):
        with pkg.Group(p, nslabs, devices=[0] * nslabs) as g:
            g.set_fields(f)
            for values, across, (lo, hi) in HELD:
                assert _same(g.section(values, across, (lo, hi)), _want(pkg, reference, "W", values, across, lo, hi)), ("group", nslabs)
                assert _same(g.section(values, across, (lo, hi), chosen), _want(pkg, reference, "W", values, across, lo, hi, chosen))
    with pkg.Solver(p) as s:  # uz at an address that is 8 mod 16
        n = int(np.prod(s.shape))
        pool = torch.zeros(n + 3, dtype=torch.float64, device="cuda")
        view = pool[1:1 + n] if pool.data_ptr() % 16 == 0 else pool[2:2 + n]
        assert view.data_ptr() % 16 == 8
        s.bind_field("uz", view.data_ptr())
        s.set_fields(f)
        for across, (lo, hi) in (("x", (0, 69)), ("x", (3, 67)), ("y", (0, 65)), ("y", (3, 65)), ("x", (69, 69))):
            assert _same(s.section(["uz"], across, (lo, hi)), _want(pkg, reference, "W", ["uz"], across, lo, hi)), ("bound", across, lo)
            assert _same(s.section(None, across, (lo, hi)), _want(pkg, reference, "W", None, across, lo, hi))
        off = (view.data_ptr() - pool.data_ptr()) // 8
        assert float(pool[:off].abs().sum()) == 0.0 and float(pool[off + n:].abs().sum()) == 0.0  # the guard elements are untouched


# ---- 5. lazy E ----------------------------------------------------------------------------------------------------

SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)


def _seeded_start(pkg, s, **knobs):
    for k, v in knobs.items():
        s.tune(k, v)
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


def test_phi_and_e_are_brought_up_to_date_and_the_moments_leave_lazy_e_alone(pkg):
    nx, ny, nz = R
    with pkg.Solver(_params(pkg, R)) as s:
        _seeded_start(pkg, s)
        s.step(3)
        uz_before = {a: s.section(["uz"], a) for a in ACROSS}
        pe = {a: s.section(["phi", "Ez"], a, (2, 9)) for a in ACROSS}
        f = s.fields()
        for a in ACROSS:
            want = np.stack([_line_sums(f[k], a, 2, 9) for k in ("phi", "Ez")])
            assert _same(pe[a], want), a
            assert _same(s.section(["uz"], a), uz_before[a]) and _same(uz_before[a][0], _line_sums(f["uz"], a, 0, (nx if a == "x" else ny) - 1))
        assert np.abs(pe["x"][1]).max() > 0.0


# ---- 6. the ring --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stride, batch, values, across, rng_, planes", [
    (1, 0, ["q", "uz"], "y", (0, 11), [1, 8, 15]),
    (3, 0, ["phi", "q"], "x", (3, 38), [8]),
    (1, 1, ["c", "q"], "x", (0, 39), [0, 2, 16]),
    (3, 1, None, "y", (4, 4), [7, 9]),
])
def test_ring_rows_equal_a_twins_synchronous_sections(pkg, stride, batch, values, across, rng_, planes):
    nx, ny, nz = R
    with pkg.Solver(_params(pkg, R)) as a, pkg.Solver(_params(pkg, R)) as b:
        _seeded_start(pkg, a, batch_moments=batch)
        _seeded_start(pkg, b)
        assert a.section_count() == (0, 0)
        a.section_arm(values, across, rng_, planes, capacity=4)
        want = []
        for k in range(1, 7):
            a.step(stride)
            a.section_record(k * stride, a.t)
            b.step(stride)
            want.append((k * stride, b.t, b.section(values, across, rng_, planes)))
        assert a.section_count() == (6, 2)  # the ring held four: the two oldest rows are gone
        steps, times, rows = a.section_read()
        assert rows.shape == (4, len(_names(pkg, values)), len(planes), ny if across == "x" else nx)
        assert steps.tolist() == [w[0] for w in want[2:]] and times.tolist() == [w[1] for w in want[2:]]
        for row, w in zip(rows, want[2:]):
            assert _same(row, w[2]), w[0]
        assert (_bits(rows[-1]) != _bits(rows[0])).any()  # the fields move
        s1, _, r1 = a.section_read(1, 2)
        assert s1.tolist() == steps[1:3].tolist() and _same(r1, rows[1:3])
        for first, count in ((2, 3), (-1, 1), (4, 1)):
            with pytest.raises(pkg.EkpnpError) as e:
                a.section_read(first, count)
            assert "status 1" in str(e.value)
        a.section_disarm()
        assert _same(a.section_read()[2], rows)
        with pytest.raises(pkg.EkpnpError):
            a.section_record(7, 0.0)
        with pytest.raises(pkg.EkpnpError) as e:
            a.section_arm(["uz"], "x", None, None, capacity=3)   # a time series needs chosen planes
        assert "nplanes = 0" in str(e.value)
        with pytest.raises(pkg.EkpnpError) as e:
            a.section_arm(["uz"], "x", None, [3], capacity=0)
        assert "capacity = 0" in str(e.value)
        a.section_arm(["uz"], "x", None, [2, 3], capacity=3)
        assert a.section_count() == (0, 0) and a.section_read()[2].shape == (0, 1, 2, ny)


# ---- 7. the ring on groups ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("nslabs, planes", [(2, [1, 8, 15]), (3, [6])])
def test_ring_on_a_group_equals_the_single_context(pkg, nslabs, planes):
    """the group steps; after every step a single context is handed the group's c, cn and uz and cut synchronously"""
    nx, ny, nz = R
    p = _params(pkg, R)
    names = ("c", "cn", "uz")
    with pkg.Group(p, nslabs, devices=[0] * nslabs) as g, pkg.Solver(p) as s:
        _seeded_start(pkg, g)
        g.section_arm(["q", "uz"], "y", (1, 10), planes, capacity=8)
        want = []
        for k in range(1, 4):
            g.step(1)
            g.section_record(k, g.t)
            for n in names:
                s.set_field(n, g.get_field(n))
            want.append(s.section(["q", "uz"], "y", (1, 10), planes))
        assert g.section_count() == (3, 0)
        steps, _, rows = g.section_read()
        assert steps.tolist() == [1, 2, 3] and rows.shape == (3, 2, len(planes), nx)
        for row, w in zip(rows, want):
            assert _same(row, w)
        assert _same(g.section(["q", "uz"], "y", (1, 10), planes), want[-1]) and _same(g.section(["q", "uz"], "y", (1, 10)), s.section(["q", "uz"], "y", (1, 10)))


def test_a_slab_without_a_chosen_plane_records_rows_of_zeros(pkg, fields, reference):
    nx, ny, nz = W
    f = fields["W"]
    p = _params(pkg, W)
    for rank, planes, expect_zero in ((2, [1, 2], True), (0, [1, 2], False), (0, [12], True), (1, [3, 5, 11], False)):
        with pkg.Solver(p, rank=rank, nranks=3, slab=True) as s:
            z0, nzl = s.z0, s.nz_local
            s.set_fields({n: v[z0:z0 + nzl] for n, v in f.items()})
            s.section_arm(["uz", "q"], "x", (3, 67), planes, capacity=2)
            s.section_record(1, 0.0)
            _, _, rows = s.section_read()
            want = _want(pkg, reference, "W", ["uz", "q"], "x", 3, 67, planes).copy()
            owned = [z0 <= z < z0 + nzl for z in planes]
            for j, own in enumerate(owned):
                if not own:
                    want[:, j, :] = 0.0
            assert (not any(owned)) == expect_zero, (rank, planes, z0, nzl)
            assert _same(rows[0], want) and (not _bits(rows[0]).any()) == expect_zero, (rank, planes)


# ---- 8. the run is left alone -----------------------------------------------------------------------------------

def test_recording_leaves_the_step_graph_and_the_run_alone(pkg):
    with pkg.Solver(_params(pkg, R)) as a, pkg.Solver(_params(pkg, R)) as b:
        _seeded_start(pkg, a)
        _seeded_start(pkg, b)
        a.step(5)
        b.step(5)
        state = a.graph_state()
        assert state == 1
        bytes_before = a.device_bytes()
        a.section_arm(["q", "uz"], "y", None, [1, 8, 15], capacity=8)
        assert a.graph_state() == state and a.device_bytes() > bytes_before
        for k in range(6):
            a.step(1)
            a.section_record(6 + k, a.t)
        b.step(6)
        assert a.graph_state() == state and b.graph_state() == state and a.section_count() == (6, 0)
        fa, fb = a.fields(), b.fields()
        for n in pkg.FIELDS:
            assert np.array_equal(_bits(fa[n]), _bits(fb[n])), n
        assert b.device_bytes() == bytes_before  # a context that never calls the new entry points allocates nothing new


# ---- 9. consistency with the plane profiles (the only toleranced check) -------------------------------------------

def test_a_full_section_adds_up_to_the_plane_sums(pkg, fields):
    nx, ny, nz = W
    f = fields["W"]
    with pkg.Solver(_params(pkg, W)) as s:
        s.set_fields(f)
        sums = s.plane_sums()
        for across in ACROSS:
            uz = s.section(["uz"], across)[0]
            q = s.section(["q"], across)[0]
            for z in range(nz):
                # each side is one summation of nx * ny terms: |error| <= (n - 1) u sum|term| each, u = 2^-53
                tol_uz = 2 * nx * ny * 2.0 ** -53 * np.abs(f["uz"][z]).sum()
                tol_q = 2 * nx * ny * 2.0 ** -53 * (np.abs(f["c"][z]).sum() + np.abs(f["cn"][z]).sum())
                d_uz = abs(math.fsum(uz[z]) - sums[pkg.PROFILE_ID["uz"], z])
                d_q = abs(math.fsum(q[z]) - (sums[pkg.PROFILE_ID["c"], z] - sums[pkg.PROFILE_ID["cn"], z]))
                print(f"across {across} z {z}: uz {d_uz:.3e} (tol {tol_uz:.3e}), q {d_q:.3e} (tol {tol_q:.3e})")
                assert d_uz <= tol_uz, (across, z, d_uz, tol_uz)
                assert d_q <= tol_q, (across, z, d_q, tol_q)


# ---- 10. the driver ---------------------------------------------------------------------------------------------

def _run_driver(args, out, code=0):
    out.mkdir()
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1", EKPNP_PLACEMENT_TRIES="1")  # the child shares device 0 with this process
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == code, (args, r.stderr[-2000:])
    return out, r.stderr


def _read_section(path, ring):
    lines = open(path).read().splitlines()
    w = lines[0].split()
    assert w[:3] == ["#", "ekpnp", "section"] and w[3:9:2] == ["nx", "ny", "nz"] and w[9:15:2] == ["across", "lo", "hi"] and w[15] == "values"
    k = w.index("nkeep")
    hdr = dict(nx=int(w[4]), ny=int(w[6]), nz=int(w[8]), across=w[10], lo=int(w[12]), hi=int(w[14]), values=w[16:k], nkeep=int(w[k + 1]))
    if ring:
        assert w[k + 2] == "planes" and w[-4] == "recorded" and w[-2] == "dropped"
        hdr.update(planes=[int(x) for x in w[k + 3:-4]], recorded=int(w[-3]), dropped=int(w[-1]))
    else:
        assert w[k + 2] == "time" and len(w) == k + 4
        hdr.update(time=float(w[k + 3]))
    rows = [ln.split() for ln in lines[1:]]
    assert all(" ".join(r) == ln for r, ln in zip(rows, lines[1:]))  # single spaces
    lead = 2 if ring else 0
    labels = [tuple(r[:lead + 2]) for r in rows]
    return hdr, labels, np.array([[float(x) for x in r[lead + 2:]] for r in rows], dtype=np.float64)


GEO = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "6", "--seed-pattern", "squares", "--seed-modes", "1,1"]


def test_driver_writes_the_rows_of_the_library_calls(pkg, tmp_path):
    assert os.path.exists(EXE), "ekpnp_main not built"
    p = pkg.default_params(40, 12, 17)
    planes, rng_ = [2, 8, 14], (1, 10)
    want, full = [], None
    with pkg.Solver(p) as s:  # the driver's loop, call by call
        s.initialization()
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-3, noise=0.0, relative=True, seed=1))
        s.fast_Poisson()
        s.init_equilibrium()
        t = 0.0
        for i in range(6):
            s.stream_collide_save(t)
            s.fast_Poisson()
            t = t + p.dt
            if (i + 1) % 2 == 0:
                want.append((i + 1, t, s.section(["q", "uz"], "y", rng_, planes)))
            if i + 1 == 3:
                s.section_write(str(tmp_path / "lib_full_3.dat"), ["q", "uz"], "y", rng_, None, time=t)
                full = s.section(["q", "uz"], "y", rng_)
    common = ["--section-values", "q,uz", "--section-across", "y", "--section-range", "1,10"]
    flags = ["--section-every", "2", *common, "--section-planes", "2,8,14"]
    plain, _ = _run_driver(GEO, tmp_path / "plain")
    loop, _ = _run_driver([*GEO, *flags], tmp_path / "loop")
    batch, _ = _run_driver([*GEO, *flags, "--batch", "1"], tmp_path / "batch")
    hdr, labels, rows = _read_section(loop / "section.dat", ring=True)
    assert hdr == dict(nx=40, ny=12, nz=17, across="y", lo=1, hi=10, values=["uz", "q"], nkeep=40, planes=planes, recorded=3, dropped=0)
    assert rows.shape == (3 * 2 * 3, 40)
    hdr0, labels0, rows0 = hdr, labels, rows
    k = 0
    for step, time, w in want:
        for vi, name in enumerate(("uz", "q")):  # ascending id, whatever the order of the flag
            for j, z in enumerate(planes):
                assert (int(labels[k][0]), float(labels[k][1]), *labels[k][2:]) == (step, time, name, str(z))
                assert np.array_equal(_bits(rows[k]), _bits(w[vi, j])), (step, name, z)  # %.17g round-trips
                k += 1
    assert (loop / "section.dat").read_bytes() == (batch / "section.dat").read_bytes()
    assert not (plain / "section.dat").exists()
    for f in ("data.dat", "umax.dat", "data_end.dat"):
        x = (plain / f).read_bytes()
        assert len(x) > 0 and x == (loop / f).read_bytes() and x == (batch / f).read_bytes(), f
    assert sorted(os.listdir(loop)) == sorted(os.listdir(plain) + ["section.dat"])
    # every plane at once: section_<step>.dat is ekpnp_section_save of the same state
    fl, _ = _run_driver([*GEO, "--section-full-every", "3", *common], tmp_path / "full")
    fb, _ = _run_driver([*GEO, "--section-full-every", "3", *common, "--batch", "1"], tmp_path / "fullbatch")
    assert sorted(os.listdir(fl)) == sorted(os.listdir(plain) + ["section_0000003.dat", "section_0000006.dat"])
    assert (fl / "section_0000003.dat").read_bytes() == (tmp_path / "lib_full_3.dat").read_bytes()
    for name in ("section_0000003.dat", "section_0000006.dat"):
        assert (fl / name).read_bytes() == (fb / name).read_bytes()
    hdr, labels, rows = _read_section(fl / "section_0000003.dat", ring=False)
    assert hdr["values"] == ["uz", "q"] and hdr["nkeep"] == 40 and labels == [(n, str(z)) for n in ("uz", "q") for z in range(17)]
    assert np.array_equal(_bits(rows.reshape(2, 17, 40)), _bits(full))
    # a group (whose slab solve rounds phi differently from a single context's) writes the same bytes with and without --batch 1
    gflags = [*GEO, *flags, "--section-full-every", "3", "--gpus", "2", "--devices", "0,0"]
    grp, _ = _run_driver(gflags, tmp_path / "group")
    grb, _ = _run_driver([*gflags, "--batch", "1"], tmp_path / "groupbatch")
    for name in ("section.dat", "section_0000003.dat", "section_0000006.dat"):
        assert (grp / name).read_bytes() == (grb / name).read_bytes(), name
    ghdr, glabels, grows = _read_section(grp / "section.dat", ring=True)
    assert ghdr == dict(hdr0, recorded=3, dropped=0) and glabels == labels0 and grows.shape == (18, 40)
    assert np.abs(grows - rows0).max() <= 1e-6 * np.abs(rows0).max()  # the same run, to the slab solve's rounding
    for bad, number in ((["--section-range", "4,12"], "hi = 12"), (["--section-planes", "3,17"], "z = 17"), (["--section-planes", "5,5"], "z = 5 after"),
                        (["--section-values", "w"], "got w"), (["--section-across", "z"], "got z")):
        _, err = _run_driver([*GEO, "--section-every", "2", *bad], tmp_path / ("bad" + "_".join(bad).replace("-", "").replace(",", "_")), code=2)
        assert number in err, err
