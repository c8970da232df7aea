"""GPU tests of the coarsened FP32 snapshots (csrc/snapshot.hip; include/ekpnp.h: ekpnp_snapshot_* and the ekpnp_group_*
spellings; `ekpnp_main --snap-every N`).

The reference below forms the block sum with the same loop of plain float64 additions the kernel is specified to make (yy
ascending outside, xx ascending inside, starting from the block's first value), divides by cx*cy and rounds once with
.astype(np.float32); z is sampled every cz-th plane.  Equality is bitwise everywhere: no tolerance appears in this file."""
import hashlib
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


def _ref(a, coarsen, z0=0):
    """a: float64 [planes z0 ..][ny][nx] -> float32 [sampled planes][ny/cy][nx/cx]"""
    cx, cy, cz = coarsen
    k0 = (z0 + cz - 1) // cz
    v = a[k0 * cz - z0::cz]
    Z, ny, nx = v.shape
    b = v.reshape(Z, ny // cy, cy, nx // cx, cx)
    S = b[:, :, 0, :, 0].copy()
    for yy in range(cy):
        for xx in range(cx):
            if yy or xx:
                S = S + b[:, :, yy, :, xx]
    return (S / float(cx * cy)).astype(np.float32)


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check(pkg, got, f, coarsen, names=None, z0=0, tag=""):
    names = list(pkg.FIELDS) if names is None else names
    assert list(got) == names, (tag, list(got))
    for n in names:
        want = _ref(f[n], coarsen, z0)
        assert _same_bits(got[n], want), (tag, n, coarsen, got[n].shape, want.shape, np.argwhere(got[n] != want)[:4])


def _random_fields(pkg, shape_zyx, seed):
    rng = np.random.default_rng(seed)
    scale = {"rho": 1000.0, "c": 30.0, "cn": 30.0, "phi": 5e-3, "T": 1.0, "Ex": 1e5, "Ey": 1e5, "Ez": 1e5}
    return {n: scale.get(n, 1e-3) * rng.uniform(-1.0, 1.0, size=shape_zyx) for n in pkg.FIELDS}


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


def _parse_vtk(path):
    """(header dict, {name: big-endian float32 [Z][Y][X]}, bytes of text, bytes of payload)"""
    raw = open(path, "rb").read()
    pos = 0

    def line():
        nonlocal pos
        e = raw.index(b"\n", pos)
        s = raw[pos:e].decode("ascii")
        pos = e + 1
        return s

    assert line() == "# vtk DataFile Version 3.0"
    title = line()
    assert len(title) < 256
    t = title.split(" ")
    assert t[:2] == ["ekpnp", "snapshot"] and t[2] == "time" and t[4:11:2] == ["nx", "ny", "nz", "coarsen"] and t[14] == "z_first", title
    h = {"time": float(t[3]), "nx": int(t[5]), "ny": int(t[7]), "nz": int(t[9]), "coarsen": tuple(int(v) for v in t[11:14]), "z_first": int(t[15])}
    assert line() == "BINARY" and line() == "DATASET STRUCTURED_POINTS"
    for key in ("DIMENSIONS", "ORIGIN", "SPACING", "POINT_DATA"):
        w = line().split(" ")
        assert w[0] == key
        h[key] = tuple(int(v) if key in ("DIMENSIONS", "POINT_DATA") else float(v) for v in w[1:])
    X, Y, Z = h["DIMENSIONS"]
    assert h["POINT_DATA"] == (X * Y * Z,)
    data, text = {}, 0
    while pos < len(raw):
        w = line().split(" ")
        assert w[0] == "SCALARS" and w[2:] == ["float", "1"], w
        assert line() == "LOOKUP_TABLE default"
        n = X * Y * Z * 4
        assert pos + n <= len(raw)
        data[w[1]] = np.frombuffer(raw, dtype=">f4", count=X * Y * Z, offset=pos).reshape(Z, Y, X)
        pos += n
    text = len(raw) - 4 * X * Y * Z * len(data)
    return h, data, text, 4 * X * Y * Z * len(data)


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


# ---- 1. block means and plane sampling -----------------------------------------------------------------

@pytest.mark.parametrize("shape, specs", [
    ((50, 8, 9), [(1, 1, 1), (2, 4, 2), (2, 8, 8), (1, 2, 4)]),   # every row ends inside a wave; X = 25 at cx = 2
    ((72, 12, 9), [(4, 4, 1), (8, 2, 2)]),
])
def test_block_means_and_plane_sampling(pkg, shape, specs):
    nx, ny, nz = shape
    p = pkg.default_params(nx, ny, nz)
    f = _random_fields(pkg, (nz, ny, nx), 7)
    with pkg.Solver(p) as s:
        s.set_fields(f)
        for co in specs:
            assert s.snapshot_planes(co[2]) == (0, (nz - 1) // co[2] + 1)  # the binding asserts the library's z_first / z_count against it
            got = s.snapshot(None, co)
            X, Y, Z, nbytes = pkg.snapshot_extent(p, None, co)
            assert got["rho"].shape == (Z, Y, X) == ((nz - 1) // co[2] + 1, ny // co[1], nx // co[0]) and nbytes == 11 * X * Y * Z * 4
            _check(pkg, got, f, co, tag=str(shape))
            if co[0] == co[1] == 1:  # z is sampled, never averaged: both plates are float32 of the plates
                for n in pkg.FIELDS:
                    assert _same_bits(got[n][0], f[n][0].astype(np.float32)) and _same_bits(got[n][-1], f[n][-1].astype(np.float32))
            three = s.snapshot(["uz", "c", "Ez"], co)  # ascending id order whatever the order asked for
            _check(pkg, three, f, co, names=["c", "uz", "Ez"], tag="mask")
            by_mask = s.snapshot((1 << 1) | (1 << 6) | (1 << 9), co)
            assert all(_same_bits(by_mask[n], three[n]) for n in three)


def test_nan_and_inf_propagate(pkg):
    nx, ny, nz = 50, 8, 9
    p = pkg.default_params(nx, ny, nz)
    f = _random_fields(pkg, (nz, ny, nx), 8)
    f["T"][2, 3, 10] = np.nan
    f["T"][4, 1, 7] = np.inf
    f["T"][4, 6, 20] = -np.inf
    with pkg.Solver(p) as s:
        s.set_fields(f)
        got = s.snapshot(["T"], (2, 4, 2))["T"]
    with np.errstate(invalid="ignore"):
        want = _ref(f["T"], (2, 4, 2))
    assert np.isnan(want[1, 0, 5]) and want[2, 0, 3] == np.inf and want[2, 1, 10] == -np.inf
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got.view(np.uint32)[ok], want.view(np.uint32)[ok])


# ---- 2. rows longer than a wave, several workgroups ------------------------------------------------------

def test_rows_longer_than_a_wave_and_several_workgroups(pkg):
    nx, ny, nz = 200, 96, 5
    p = pkg.default_params(nx, ny, nz)
    f = _random_fields(pkg, (nz, ny, nx), 11)
    with pkg.Solver(p) as s:
        s.set_fields(f)
        for co in [(2, 2, 1), (8, 8, 4)]:
            _check(pkg, s.snapshot(None, co), f, co, tag="200x96x5")


# ---- 3. a caller-bound field that is only 8-byte aligned -------------------------------------------------

def test_bound_field_at_an_8_byte_aligned_address(pkg):
    import torch

    nx, ny, nz = 72, 12, 9
    p = pkg.default_params(nx, ny, nz)
    f = _random_fields(pkg, (nz, ny, nx), 13)
    with pkg.Solver(p) as s:
        n = int(np.prod(s.shape))
        pool = torch.zeros(n + 3, dtype=torch.float64, device="cuda")
        view = pool[1:1 + n] if pool.data_ptr() % 16 == 0 else pool[2:2 + n]
        assert view.data_ptr() % 16 == 8
        s.bind_field("uz", view.data_ptr())
        s.set_fields(f)
        assert s.field_device_ptr("uz") == view.data_ptr()
        for co in [(2, 2, 1), (4, 1, 2), (8, 4, 1)]:
            _check(pkg, s.snapshot(["uy", "uz", "T"], co), f, co, names=["uy", "uz", "T"], tag="bound")
        assert float(pool[0]) == 0.0 and float(pool[-1]) == 0.0


# ---- 4. a running lattice ---------------------------------------------------------------------------------

@pytest.mark.parametrize("batch_moments", [0, 1])
def test_snapshot_of_a_running_lattice(pkg, O, batch_moments):
    co = (2, 2, 4)
    with _perturbed_run(pkg, O, (40, 12, 17), 0, batch_moments=batch_moments) as s:
        s.step(12)  # the last solve was lazy: nothing has looked at phi or E since
        first = s.snapshot(["Ex", "phi"], co)
        everything = s.snapshot(None, co)
        f = s.fields()
        _check(pkg, first, f, co, names=["phi", "Ex"], tag="lazy")
        _check(pkg, everything, f, co, tag="running")
        assert np.abs(first["Ex"]).max() > 0.0 and np.abs(everything["uz"]).max() > 0.0
        s.fast_Poisson()  # ... and right after a solve on its own
        again = s.snapshot(["Ex", "phi"], co)
        _check(pkg, again, s.fields(), co, names=["phi", "Ex"], tag="after fast_Poisson")


# ---- 5. independent of the decomposition ------------------------------------------------------------------

def test_snapshots_do_not_depend_on_the_decomposition(pkg, tmp_path):
    nx, ny, nz = 40, 12, 17
    p = pkg.default_params(nx, ny, nz)
    f = _random_fields(pkg, (nz, ny, nx), 5)
    specs = [(2, 2, 4), (4, 1, 8), (1, 1, 1)]
    ref, sha = {}, {}
    with pkg.Solver(p) as s:
        s.set_fields(f)
        for co in specs:
            ref[co] = s.snapshot(None, co)
            _check(pkg, ref[co], f, co, tag="two-buffer")
            path = tmp_path / ("one_%d%d%d.vtk" % co)
            s.snapshot_begin(str(path), None, co, time=0.125)
            s.snapshot_finish()
            sha[co] = _sha(path)
    pi = p.copy()
    pi.in_place = 1
    with pkg.Solver(pi) as s:
        s.set_fields(f)
        for co in specs:
            got = s.snapshot(None, co)
            assert all(_same_bits(got[n], ref[co][n]) for n in pkg.FIELDS), ("in place", co)
            path = tmp_path / ("inplace_%d%d%d.vtk" % co)
            s.snapshot_begin(str(path), None, co, time=0.125)
            s.snapshot_finish()
            assert _sha(path) == sha[co]
    for nslabs in (2, 3, 4):
        with pkg.Group(p, nslabs, devices=[0] * nslabs) as g:
            if nslabs == 4:  # with cz = 8 (planes 0, 8, 16) the second slab holds no sampled plane
                assert [g.slab_extent(i) for i in range(4)] == [(0, 4), (4, 4), (8, 4), (12, 5)]
            g.set_fields(f)
            for co in specs:
                got = g.snapshot(None, co)
                assert all(_same_bits(got[n], ref[co][n]) for n in pkg.FIELDS), (nslabs, co)
                path = tmp_path / ("group%d_%d%d%d.vtk" % ((nslabs,) + co))
                g.snapshot_begin(str(path), None, co, time=0.125)
                assert g.snapshot_pending == 1
                g.snapshot_finish()
                assert g.snapshot_pending == 0 and _sha(path) == sha[co], (nslabs, co)
            three = g.snapshot(["T", "rho"], (2, 2, 4))
            assert list(three) == ["rho", "T"] and all(_same_bits(three[n], ref[(2, 2, 4)][n]) for n in three)
    # stand-alone slab contexts write their own planes, the title and ORIGIN saying where they sit
    with pkg.Solver(p, rank=0, nranks=1, slab=True) as s:
        s.set_fields(f)
        co = (2, 2, 4)
        got = s.snapshot(None, co)
        assert all(_same_bits(got[n], ref[co][n]) for n in pkg.FIELDS)
        s.snapshot_begin(str(tmp_path / "slab1.vtk"), None, co, time=0.125)
        s.snapshot_finish()
        h, _, _, _ = _parse_vtk(tmp_path / "slab1.vtk")
        assert h["z_first"] == 0 and _sha(tmp_path / "slab1.vtk") == sha[co]
    for rank in range(2):
        with pkg.Solver(p, rank=rank, nranks=2, slab=True) as s:
            z0, nzl = s.z0, s.nz_local
            assert (z0, nzl) == ((0, 8), (8, 9))[rank]
            s.set_fields({n: v[z0:z0 + nzl] for n, v in f.items()})
            for co in [(2, 2, 4), (4, 1, 8)]:
                k0, kn = s.snapshot_planes(co[2])
                got = s.snapshot(None, co)
                assert all(_same_bits(got[n], ref[co][n][k0:k0 + kn]) for n in pkg.FIELDS), (rank, co)
                path = tmp_path / ("rank%d_%d.vtk" % (rank, co[2]))
                s.snapshot_begin(str(path), ["uz"], co, time=0.5)
                s.snapshot_finish()
                h, data, _, _ = _parse_vtk(path)
                assert h["z_first"] == k0 and h["DIMENSIONS"] == (nx // co[0], ny // co[1], kn)
                assert h["ORIGIN"][2] == k0 * co[2] * p.dz
                assert _same_bits(data["uz"].astype(np.float32), ref[co]["uz"][k0:k0 + kn])
    # a slab that holds no sampled plane: zero planes in memory, no file, EKPNP_OK
    with pkg.Solver(p, rank=1, nranks=4, slab=True) as s:
        assert (s.z0, s.nz_local) == (4, 4) and s.snapshot_planes(8) == (1, 0)
        got = s.snapshot(["uz"], (2, 2, 8))
        assert got["uz"].shape == (0, 6, 20)
        s.snapshot_begin(str(tmp_path / "empty.vtk"), None, (2, 2, 8))
        s.snapshot_finish()
        assert not (tmp_path / "empty.vtk").exists() and s.snapshot_pending == 0


# ---- 6. ordering --------------------------------------------------------------------------------------------

def test_a_snapshot_is_of_the_state_at_begin_whatever_is_enqueued_after_it(pkg, O, tmp_path):
    shape, co = (40, 12, 17), (2, 2, 4)
    with _perturbed_run(pkg, O, shape, 3) as a, _perturbed_run(pkg, O, shape, 3) as b:
        a.snapshot_begin(str(tmp_path / "a.vtk"), None, co, time=1.5)  # stream order decides what it holds, not timing
        assert a.snapshot_pending == 1
        a.step(5)
        a.snapshot_finish()
        assert a.snapshot_pending == 0
        b.snapshot_begin(str(tmp_path / "b.vtk"), None, co, time=1.5)
        b.snapshot_finish()
        b.step(5)
        assert (tmp_path / "a.vtk").read_bytes() == (tmp_path / "b.vtk").read_bytes()
        fa, fb = a.fields(), b.fields()
        for n in pkg.FIELDS:  # a snapshot in flight does not disturb the run
            assert np.array_equal(fa[n], fb[n]), n


def test_three_begins_in_a_row_and_destroy_with_one_pending(pkg, O, tmp_path):
    shape, co = (40, 12, 17), (2, 2, 4)
    X, Y, Z, payload = pkg.snapshot_extent(pkg.default_params(*shape), ["uz", "c", "cn"], co)
    with _perturbed_run(pkg, O, shape, 2) as a, _perturbed_run(pkg, O, shape, 2) as b:
        base = a.device_bytes()
        want = []
        for i in range(3):
            a.snapshot_begin(str(tmp_path / f"s{i}.vtk"), ["uz", "c", "cn"], co, time=float(i))
            assert a.snapshot_pending == min(i + 1, 2)  # the third begin first finishes the oldest
            assert a.device_bytes() == base + min(i + 1, 2) * payload  # two staging slots, made when first used, counted
            a.step(2)
            want.append(b.snapshot(["uz", "c", "cn"], co))
            b.step(2)
        assert (tmp_path / "s0.vtk").exists() and not (tmp_path / "s2.vtk").exists()
        a.snapshot_finish()
        assert a.snapshot_pending == 0
        for i in range(3):
            h, data, _, _ = _parse_vtk(tmp_path / f"s{i}.vtk")
            assert h["time"] == float(i) and list(data) == ["c", "cn", "uz"]
            for n in data:
                assert _same_bits(data[n].astype(np.float32), want[i][n]), (i, n)
        assert not np.array_equal(want[0]["uz"], want[2]["uz"])  # the three states differ
        a.snapshot_begin(str(tmp_path / "never.vtk"), ["uz", "c", "cn"], co)
        a.step(1)
        assert a.snapshot_pending == 1 and a.device_bytes() == base + 2 * payload  # nothing grows: slots are re-used
    # left the with block with one pending: ekpnp_destroy discarded it without hanging and without a file
    assert not (tmp_path / "never.vtk").exists()


# ---- 7. the file ------------------------------------------------------------------------------------------------

def test_file_is_legacy_vtk_with_big_endian_floats(pkg, O, tmp_path):
    shape, co = (40, 12, 17), (4, 2, 8)
    with _perturbed_run(pkg, O, shape, 4) as s:
        path = tmp_path / "snap.vtk"
        s.snapshot_begin(str(path), None, co, time=s.t)
        s.snapshot_finish()
        mem = s.snapshot(None, co)
        p, t = s.p, s.t
    h, data, text, payload = _parse_vtk(path)
    X, Y, Z, nbytes = pkg.snapshot_extent(p, None, co)
    assert (h["nx"], h["ny"], h["nz"], h["coarsen"], h["z_first"], h["time"]) == (40, 12, 17, co, 0, t)
    assert h["DIMENSIONS"] == (X, Y, Z) == (10, 6, 3)
    assert h["ORIGIN"] == ((co[0] - 1) * p.dx / 2, (co[1] - 1) * p.dy / 2, 0.0)
    assert h["SPACING"] == (co[0] * p.dx, co[1] * p.dy, co[2] * p.dz)
    assert list(data) == pkg.FIELDS
    for n in pkg.FIELDS:
        assert _same_bits(data[n].astype(np.float32), mem[n]), n
    assert payload == nbytes and os.path.getsize(path) == text + nbytes
    expected_text = sum(len(line) + 1 for line in open(path, "rb").read().split(b"\n")[:8]) + sum(len(f"SCALARS {n} float 1\nLOOKUP_TABLE default\n") for n in pkg.FIELDS)
    assert text == expected_text  # header and per-field lines only: nothing else in the file


# ---- 8. errors --------------------------------------------------------------------------------------------------

def test_errors_leave_the_context_usable(pkg, tmp_path):
    import ctypes as C

    nx, ny, nz = 50, 8, 51
    p = pkg.default_params(nx, ny, nz)
    f = _random_fields(pkg, (nz, ny, nx), 3)
    lib = pkg.load_library()
    with pkg.Solver(p) as s:
        s.set_fields(f)
        buf = np.empty(11 * nz * ny * nx, dtype=np.float32)
        a, b = C.c_int(), C.c_int()
        for fields, co, number in [(None, (3, 1, 1), "3"), (None, (4, 1, 1), "50"), (None, (1, 1, 4), "50"), (1 << 11, (1, 1, 1), "2048")]:
            spec = pkg.snapshot_spec(fields, co)
            assert lib.ekpnp_snapshot_read(s.handle, C.byref(spec), buf.ctypes.data_as(C.c_void_p), C.byref(a), C.byref(b)) == 1
            assert number in lib.ekpnp_last_error(s.handle).decode()
            assert lib.ekpnp_snapshot_begin(s.handle, C.byref(spec), os.fsencode(str(tmp_path / "bad.vtk")), 0.0) == 1
            assert number in lib.ekpnp_last_error(s.handle).decode()
            with pytest.raises(pkg.EkpnpError):
                s.snapshot(fields, co)
        assert s.snapshot_pending == 0 and not (tmp_path / "bad.vtk").exists()
        # the file is opened at finish: that is where a path that cannot be opened is reported
        s.snapshot_begin(str(tmp_path / "no_such_directory" / "x.vtk"), None, (2, 2, 2))
        assert s.snapshot_pending == 1
        with pytest.raises(pkg.EkpnpError) as e:
            s.snapshot_finish()
        assert "cannot open" in str(e.value) and s.snapshot_pending == 0
        s.snapshot_begin(str(tmp_path / "good.vtk"), None, (2, 2, 2))
        s.snapshot_finish()
        _, data, _, _ = _parse_vtk(tmp_path / "good.vtk")
        assert _same_bits(data["T"].astype(np.float32), _ref(f["T"], (2, 2, 2)))
        _check(pkg, s.snapshot(None, (2, 2, 2)), f, (2, 2, 2), tag="after errors")
    with pkg.Group(p, 2, devices=[0, 0]) as g:
        g.set_fields(f)
        with pytest.raises(pkg.EkpnpError) as e:
            g.snapshot(None, (1, 1, 4))
        assert "50" in str(e.value)
        g.snapshot_begin(str(tmp_path / "no_such_directory" / "g.vtk"), None, (2, 2, 2))
        with pytest.raises(pkg.EkpnpError):
            g.snapshot_finish()
        assert g.snapshot_pending == 0
        _check(pkg, g.snapshot(None, (2, 2, 2)), f, (2, 2, 2), tag="group after errors")


# ---- 9. the driver ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gpus", [1, 2])
def test_driver_writes_a_snapshot_every_n_iterations(pkg, tmp_path, gpus):
    assert os.path.exists(EXE), "ekpnp_main not built"
    out = tmp_path / "out"
    out.mkdir()
    args = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "12", "--snap-every", "6", "--snap-coarsen", "2,2,4", "--snap-fields", "uz,c,cn"]
    if gpus > 1:
        args += ["--gpus", str(gpus)]
    r = subprocess.run([EXE, *args, "--out", str(out)], capture_output=True, text=True, timeout=300)  # a fresh child process under a time limit
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(f for f in os.listdir(out) if f.startswith("snap_")) == ["snap_0000006.vtk", "snap_0000012.vtk"]
    # the same run in this process: the driver's call sequence (main.cu:161-200)
    p = pkg.default_params(40, 12, 17)
    with (pkg.Solver(p) if gpus == 1 else pkg.Group(p, gpus, devices=[0] * gpus)) as s:
        s.initialization()
        s.init_equilibrium()
        t = 0.0
        mid = None
        for i in range(12):
            s.stream_collide_save(t)
            s.fast_Poisson()
            t = t + p.dt
            if i == 5:
                mid = s.snapshot(["uz", "c", "cn"], (2, 2, 4))
        last = s.snapshot(["uz", "c", "cn"], (2, 2, 4))
    for name, want in (("snap_0000006.vtk", mid), ("snap_0000012.vtk", last)):
        h, data, _, _ = _parse_vtk(out / name)
        assert h["coarsen"] == (2, 2, 4) and h["DIMENSIONS"] == (20, 6, 5) and list(data) == ["c", "cn", "uz"]
        for n in data:
            assert _same_bits(data[n].astype(np.float32), want[n]), (name, n)
    assert _parse_vtk(out / "snap_0000012.vtk")[0]["time"] == t
    assert np.abs(last["c"]).max() > 0.0
