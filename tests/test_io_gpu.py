"""GPU tests of the §8(f) rows: on-device diagnostics and the main.cu IO surface.
The writers are checked BYTE FOR BYTE against files written by the reference's own
save_data_tecplot / save_data_end / record_umax (sha256 in tests/golden/ref_g6.npz, produced by
oracle/_ref/ref_driver in `io` mode on seeded fields)."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

from conftest import golden_path

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mirror(pkg, po):
    p = pkg.Params()
    for name, _ in p._fields_:
        setattr(p, name, getattr(po, name))
    return p


def _io_fields():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.io_fields()


def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def test_current_and_umax_on_device_vs_oracle(pkg, O):
    po = O.default_params(40, 12, 17)
    po.pb_iterations = 20
    orc = O.Oracle(po)
    orc.initialization()
    start = O.perturb_fields(po, orc.fields())
    orc.set_fields(start); orc.fast_poisson(); orc.init_equilibrium(); orc.step(12)
    with pkg.Solver(_mirror(pkg, po)) as s:
        s.initialization(); s.set_fields(start); s.fast_Poisson(); s.init_equilibrium(); s.step(12)
        cur, um = s.current(), s.umax()
        # and on exactly the oracle's fields: only the summation order differs
        s.set_fields(orc.fields())
        cur2, um2 = s.current(), s.umax()
    assert abs(cur2 - orc.current()) <= 1e-13 * abs(orc.current())
    assert um2 == orc.umax()
    assert abs(cur - orc.current()) <= 1e-9 * abs(orc.current())
    assert abs(um - orc.umax()) <= 1e-7 * abs(orc.umax())


def test_umax_is_zero_when_nothing_moves_up(pkg):
    p = pkg.default_params(16, 4, 8)
    with pkg.Solver(p) as s:
        s.set_field("uz", -np.ones(s.shape))
        assert s.umax() == 0.0  # LBM.cu:2718: umax starts at 0


def test_writers_byte_compatible_with_the_reference(pkg, O, tmp_path):
    g = np.load(golden_path("ref_g6.npz")) if os.path.exists(golden_path("ref_g6.npz")) else None
    if g is None:
        pytest.skip("ref_g6.npz missing")
    f = _io_fields()
    raw = np.concatenate([np.ascontiguousarray(f[k], dtype=np.float64).ravel() for k in O.FIELDS]).tobytes()
    if hashlib.sha256(raw).hexdigest() != str(g["input_sha256"]):
        pytest.skip("numpy's random stream differs from the one the golden was made with")
    po = O.default_params(50, 8, 51)
    po.Lx, po.Ly, po.Lz = 0.5e-6, 0.08e-6, 0.5e-6
    with pkg.Solver(_mirror(pkg, po)) as s:
        s.set_fields(f)
        d = str(tmp_path / "data.dat")
        s.save_data_tecplot(d, 1.25e-8, first=True, append=False)
        s.save_data_tecplot(d, 2.5e-8, first=False, append=True)
        e = str(tmp_path / "data_end.dat")
        s.save_data_end(e, 1.25e-8)
        u = str(tmp_path / "umax.dat")
        s.record_umax(u, 1.25e-8, append=False)
        cur = s.current()
        for name, path in (("data.dat", d), ("data_end.dat", e), ("umax.dat", u)):
            assert os.path.getsize(path) == int(g[name + "_size"]), name
            head = "\n".join(open(path).read().split("\n")[:6])
            assert head == str(g[name + "_head"]), name
            assert _sha(path) == str(g[name + "_sha256"]), name
        assert abs(cur - float(g["current"])) <= 1e-13 * abs(float(g["current"]))
        # read_data (LBM.cu:2632-2671) on that byte-identical restart file
        with pkg.Solver(_mirror(pkg, po)) as r:
            t = r.read_data(e)
            assert t == float("%10.6f" % 1.25e-8)
            ext = {k: np.array(v, copy=True) for k, v in f.items()}
            for k in ("rho", "c", "cn", "ux", "uy", "uz"):  # the writer extrapolates these to the walls
                ext[k][0] = 2 * ext[k][1] - ext[k][2]
                ext[k][-1] = 2 * ext[k][-2] - ext[k][-3]
            for k in O.FIELDS:
                want = np.array([float("%10.6f" % v) for v in ext[k].ravel()]).reshape(ext[k].shape)
                assert np.array_equal(r.get_field(k), want), k


def test_io_errors_are_returned(pkg, tmp_path):
    p = pkg.default_params(8, 4, 6)
    with pkg.Solver(p) as s:
        with pytest.raises(pkg.EkpnpError):
            s.read_data(str(tmp_path / "missing.dat"))
        (tmp_path / "short.dat").write_text("0 0 0 0 0 0 0 0 0 0 0 0\n")
        with pytest.raises(pkg.EkpnpError):
            s.read_data(str(tmp_path / "short.dat"))
        with pytest.raises(pkg.EkpnpError):
            s.save_data_end(str(tmp_path / "no_such_dir" / "x.dat"), 0.0)


# ---- §8(f) row 4: PB initialisation with a convergence test ---------------------------------

def test_initialization_converged_matches_fixed_sweeps_on_the_reference_grid(pkg, O):
    po = O.default_params(50, 8, 51)
    po.Lx, po.Ly, po.Lz = 0.5e-6, 0.08e-6, 0.5e-6
    p = _mirror(pkg, po)
    with pkg.Solver(p) as a, pkg.Solver(p) as b:
        a.initialization()
        n, res = b.initialization_converged(rel_tol=0.0, max_sweeps=501)
        assert n == 501, (n, res)
        for k in ("phi", "c", "cn", "Ez", "T", "rho"):
            assert np.array_equal(a.get_field(k), b.get_field(k)), k
        n2, res2 = b.initialization_converged(rel_tol=1e-9, max_sweeps=20000)
        assert res2 <= 1e-9 and n2 < 501  # 320 sweeps: the fixed 501 of LBM.cu:89 over-iterate
        assert np.abs(b.get_field("phi") - a.get_field("phi")).max() < 1e-8 * abs(po.voltage)
        c, cn = b.get_field("c"), b.get_field("cn")
        assert np.allclose(c * cn, po.chargeinf**2, rtol=1e-12)


def test_initialization_converged_on_a_tall_channel_where_the_reference_diverges(pkg, O):
    """NZ = 256: (Lz/(pi lambda_D))^2 = 78, the reference's PB_omega = 0.05 diverges (NaN)."""
    p = pkg.default_params(16, 8, 256)
    with pkg.Solver(p) as s:
        s.initialization()
        assert not np.isfinite(s.get_field("phi")).all()  # the reference's own start-up blows up here
        n, res = s.initialization_converged(rel_tol=1e-8, max_sweeps=50000)
        f = s.fields()
        assert res <= 1e-8 and all(np.isfinite(v).all() for v in f.values())
        assert np.allclose(f["c"] * f["cn"], p.chargeinf**2, rtol=1e-10)
        mid = f["phi"][128, 0, 0]
        assert abs(mid) < 1e-5 * abs(p.voltage)  # double layers 14 Debye lengths from the mid-plane: neutral core
        # Gouy-Chapman at the wall: tanh(e phi/4kT) = tanh(e zeta/4kT) exp(-z/lambda_D), lattice value within 2 %
        lam = np.sqrt(p.eps * p.kB * p.roomT / p.electron / (2 * p.chargeinf * p.convertCtoCharge))
        vt = p.kB * p.roomT / p.electron
        z = 5 * p.dz
        gc = 4 * vt * np.arctanh(np.tanh(p.voltage / (4 * vt)) * np.exp(-z / lam))
        assert abs(f["phi"][5, 0, 0] - gc) < 0.02 * abs(gc)


# ---- the C++ host that keeps main.cu's driver / IO surface -------------------------------------

def test_cpp_driver_reproduces_the_library_calls(pkg, O, tmp_path):
    """ek-pnp-3d_amd/ekpnp_main (csrc/ekpnp_main.cpp) runs main.cu's sequence over the C ABI; its
    files must be byte-identical to the same sequence driven through the ctypes mirror."""
    import subprocess

    exe = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
    if not os.path.exists(exe):
        pytest.skip("ekpnp_main not built")
    shape, steps, nsave, pc = (16, 8, 17), 60, 20, 10
    out = tmp_path / "cpp"
    out.mkdir()
    r = subprocess.run([exe, "--nx", str(shape[0]), "--ny", str(shape[1]), "--nz", str(shape[2]), "--steps", str(steps), "--nsave", str(nsave),
                        "--print-current", str(pc), "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "speed:" in r.stdout and r.stdout.count("Current = ") == steps // pc
    p = pkg.default_params(*shape)
    ref = tmp_path / "py"
    ref.mkdir()
    currents = []
    with pkg.Solver(p) as s:
        s.initialization(); s.init_equilibrium()
        t = 0.0
        s.save_data_tecplot(str(ref / "data.dat"), t, first=True, append=False)
        open(ref / "umax.dat", "wb").close()
        for i in range(steps):  # main.cu:189-224
            s.stream_collide_save(t); s.fast_Poisson(); t = t + p.dt
            if i % nsave == 1:
                s.save_data_tecplot(str(ref / "data.dat"), t, first=True, append=True)
            if i % pc == 1:
                currents.append(s.current())
                s.record_umax(str(ref / "umax.dat"), t, append=True)
        s.save_data_tecplot(str(ref / "data.dat"), t, first=True, append=True)
        s.save_data_end(str(ref / "data_end.dat"), t)
    for name in ("data.dat", "umax.dat", "data_end.dat"):
        assert _sha(str(out / name)) == _sha(str(ref / name)), name
    printed = [float(l.split("Current = ")[1]) for l in r.stdout.splitlines() if "Current = " in l]
    assert np.allclose(printed, currents, rtol=1e-5)  # %g prints 6 significant digits
    # restart: main.cu:161-164 (flag == 1) reads data_end.dat back
    r2 = subprocess.run([exe, "--nx", str(shape[0]), "--ny", str(shape[1]), "--nz", str(shape[2]), "--steps", "2", "--read-previous", "1",
                         "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and "Reading previous data" in r2.stdout, r2.stderr
    # ... and the lossless variant: write data_end.bin, restart from it
    geo = ["--nx", str(shape[0]), "--ny", str(shape[1]), "--nz", str(shape[2]), "--out", str(out)]
    r4 = subprocess.run([exe, *geo, "--steps", "4", "--binary-state", "1"], capture_output=True, text=True, timeout=300)
    assert r4.returncode == 0 and os.path.getsize(out / "data_end.bin") == 40 + 11 * 8 * shape[0] * shape[1] * shape[2], r4.stderr
    r5 = subprocess.run([exe, *geo, "--steps", "2", "--read-previous", "2"], capture_output=True, text=True, timeout=300)
    assert r5.returncode == 0 and "(binary)" in r5.stdout, r5.stderr
    r3 = subprocess.run([exe, "--nx", "8", "--ny", "8", "--nz", "2"], capture_output=True, text=True, timeout=60)
    assert r3.returncode != 0 and "failed" in r3.stderr  # errors are reported, never a crash


def test_save_scalar_names_and_bytes(pkg, tmp_path):
    """save_scalar, LBM.cu:2454-2490: "<name><n padded to the digits of NSTEPS>.bin", raw FP64."""
    p = pkg.default_params(12, 6, 8)
    with pkg.Solver(p) as s:
        a = np.arange(12 * 6 * 8, dtype=np.float64).reshape(s.shape)
        s.set_field("ux", a)
        s.save_scalar(str(tmp_path / "ux"), "ux", 37, nsteps=1000)
        assert np.array_equal(np.fromfile(tmp_path / "ux0037.bin"), a.ravel())
        s.save_scalar(str(tmp_path / "ux"), "ux", 5, nsteps=99)
        assert (tmp_path / "ux05.bin").exists()


def test_copy_bandwidth_probe(pkg):
    """ekpnp_copy_bandwidth: the measured streaming ceiling bench.py reports next to the 8 TB/s
    spec figure.  A 256 MiB copy on an MI355X is far above 500 GB/s and cannot exceed the spec."""
    p = pkg.default_params(16, 8, 9)
    with pkg.Solver(p) as s:
        bw = s.copy_bandwidth(256 << 20)
        assert 500.0 < bw < 8000.0, bw
        with pytest.raises(pkg.EkpnpError):
            s.copy_bandwidth(0)


def test_binary_state_is_lossless(pkg, O, tmp_path):
    """ekpnp_save_state / ekpnp_read_state ("lossless binary variant"): the 11
    fields come back bit for bit, the run restarted from the file (read_state + init_equilibrium,
    main.cu:161-175) continues exactly like one restarted from the same fields in memory, and the
    reference's text file (6 decimals) does not."""
    po = O.default_params(20, 6, 11)
    po.pb_iterations = 5
    p = pkg.Params()
    for n, _ in p._fields_:
        setattr(p, n, getattr(po, n))
    path = str(tmp_path / "state.bin")
    with pkg.Solver(p) as s:
        s.initialization()
        s.set_fields(O.perturb_fields(po, s.fields())); s.fast_Poisson(); s.init_equilibrium()
        s.step(7)
        saved = s.fields()
        s.save_state(path, 7 * p.dt)
        s.save_data_end(str(tmp_path / "data_end.dat"), 7 * p.dt)
        s.init_equilibrium(); s.step(3)          # restart in memory: fields -> equilibrium -> run on
        want = s.fields()
    assert os.path.getsize(path) == 40 + 11 * 8 * 20 * 6 * 11
    with pkg.Solver(p) as s:
        t = s.read_state(path)
        assert t == 7 * p.dt
        got = s.fields()
        for k in saved:
            assert np.array_equal(got[k], saved[k]), k
        s.init_equilibrium(); s.step(3)
        cont = s.fields()
        for k in want:
            assert np.array_equal(cont[k], want[k]), k
    with pkg.Solver(p) as s:
        s.read_data(str(tmp_path / "data_end.dat"))
        assert not np.array_equal(s.get_field("phi"), saved["phi"])  # the text format is lossy
    q = p.copy(); q.nz = 12; q.Lz = (q.nz - 1) * q.dz
    with pkg.Solver(q) as s:
        with pytest.raises(pkg.EkpnpError):
            s.read_state(path)                   # written for a different lattice


def test_cpp_driver_converged_start_on_a_tall_channel(pkg, tmp_path):
    """The reference's initialization() - 501 Picard sweeps with PB_omega = 0.05, LBM.cu:89-106 - diverges to NaN on channels
    taller than about 180 planes at the default spacing (the reference itself would, too); `ekpnp_main --converged-init TOL`
    starts from ekpnp_initialization_converged instead, also over a group of slabs."""
    import subprocess

    exe = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
    if not os.path.exists(exe):
        pytest.skip("ekpnp_main not built")
    geo = ["--nx", "16", "--ny", "8", "--nz", "257", "--steps", "12", "--print-current", "5"]
    bad = subprocess.run([exe, *geo, "--out", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 0 and "Current = nan" in bad.stdout.replace("-nan", "nan"), bad.stdout[-500:]
    for extra in ([], ["--devices", "0,0"]):
        ok = subprocess.run([exe, *geo, "--converged-init", "1e-9", "--out", str(tmp_path), *extra], capture_output=True, text=True, timeout=300)
        assert ok.returncode == 0, ok.stderr
        assert "Poisson-Boltzmann start-up:" in ok.stdout and "nan" not in ok.stdout.lower(), ok.stdout[-800:]
        cur = [float(l.split("Current = ")[1]) for l in ok.stdout.splitlines() if "Current = " in l]
        assert len(cur) == 3 and all(np.isfinite(cur)) and all(abs(c) > 0 for c in cur)


def test_a_rejected_kernel_launch_is_reported_by_name(tmp_path):
    """Every launch is checked (note_launch): the entry point returns EKPNP_ERR_HIP and
    ekpnp_last_error names the kernel.  Driven by the library's fault-injection knob in a child
    process (the knob is read once); EKPNP_DEBUG_SYNC=1 (synchronise after every launch) must give
    the same fields as a normal run."""
    import subprocess
    import sys

    code = r'''
import sys, numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as G
pkg = G.load_package()
import os
p = pkg.default_params(int(os.environ.get("EKPNP_TEST_NX", "16")), int(os.environ.get("EKPNP_TEST_NY", "8")), int(os.environ.get("EKPNP_TEST_NZ", "12"))); p.pb_iterations = 3
with pkg.Solver(p) as s:
    try:
        s.initialization(); s.init_equilibrium(); s.step(2)
        np.save(sys.argv[1], s.get_field("rho"))
        print("OK", pkg.load_library().ekpnp_debug_sync_enabled())
    except pkg.EkpnpError as e:
        print("ERR", e)
''' % ROOT
    def run(env_extra, out):
        env = dict(os.environ, **env_extra)
        return subprocess.run([sys.executable, "-c", code, str(out)], env=env, capture_output=True, text=True, timeout=300)

    # (the eleven child processes run four at a time: each is a second of HIP start-up around microseconds of kernels)
    from concurrent.futures import ThreadPoolExecutor

    cases = [({"EKPNP_INJECT_LAUNCH_FAILURE": "k_pbe_relax"}, "k_pbe_relax"),
             ({"EKPNP_INJECT_LAUNCH_FAILURE": "k_collide_all"}, "k_collide_all"),  # small lattice: plates + bulk in one launch
             ({"EKPNP_INJECT_LAUNCH_FAILURE": "k_collide_bulk", "EKPNP_NO_MERGED_WALLS": "1"}, "k_collide_bulk")]
    # the z solve has six kernels; each launch is noted under the name of the kernel that was really launched.  The 8 x 7
    # plane has 56 modes (nxh = 8), not a multiple of 16: its 129-row columns take <4> where the 16 x 8 plane's take <8,32>
    for nz, knob, kernel, (nx, ny) in (("12", "1", "k_tridiag_pcr64", (16, 8)), ("300", "2", "k_tridiag_part<8>", (16, 8)),
                                       ("131", "2", "k_tridiag_part<8,32>", (16, 8)), ("100", "2", "k_tridiag_part<8,16>", (16, 8)),
                                       ("131", "2", "k_tridiag_part<4>", (8, 7)), ("300", "0", "k_tridiag", (16, 8))):
        cases.append(({"EKPNP_INJECT_LAUNCH_FAILURE": kernel, "EKPNP_TEST_NX": str(nx), "EKPNP_TEST_NY": str(ny), "EKPNP_TEST_NZ": nz,
                       "EKPNP_TRI_PARTITION": knob}, kernel))
    with ThreadPoolExecutor(max_workers=4) as pool:
        results = list(pool.map(lambda c: run(c[0], tmp_path / ("x_%d.npy" % cases.index(c))), cases))
        a, b = pool.map(lambda eo: run(*eo), [({}, tmp_path / "a.npy"), ({"EKPNP_DEBUG_SYNC": "1"}, tmp_path / "b.npy")])
    for (env_extra, kernel), r in zip(cases, results):
        assert r.returncode == 0 and "ERR" in r.stdout and f"kernel {kernel}" in r.stdout, (kernel, r.stdout, r.stderr[-2000:])
        if "tridiag" in kernel:
            assert f"kernel {kernel}:" in r.stdout, (kernel, r.stdout)
    assert "OK 0" in a.stdout and "OK 1" in b.stdout, (a.stdout, b.stdout, b.stderr[-2000:])
    assert np.array_equal(np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy"))


def test_restart_reequilibrates_like_the_reference(pkg, O, tmp_path):
    """What 'restart' means here and in the reference (main.cu:161-175): read the fields, then
    init_equilibrium.  The state file keeps the fields bit for bit, but the non-equilibrium part of
    the populations is not stored, so the restarted run differs from the uninterrupted one - by a
    small, bounded amount that this test documents - and is deterministic."""
    po = O.default_params(20, 6, 21)
    po.pb_iterations = 10
    p = pkg.default_params(20, 6, 21)
    p.pb_iterations = 10
    with pkg.Solver(p) as s:
        s.initialization()
        s.set_fields(O.perturb_fields(po, s.fields()))
        s.fast_Poisson(); s.init_equilibrium(); s.step(30)
        s.save_state(str(tmp_path / "s.bin"), s.t)
        at_save = s.fields()
        s.step(30)
        straight = s.fields()
    runs = []
    for _ in range(2):
        with pkg.Solver(p) as s:
            t = s.read_state(str(tmp_path / "s.bin"))
            assert abs(t - 30 * p.dt) < 1e-20
            got = s.fields()
            for k in at_save:
                assert np.array_equal(got[k], at_save[k]), k  # the fields come back bit for bit
            s.init_equilibrium()
            s.step(30)
            runs.append(s.fields())
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k       # deterministic
    err = O.rel_l2(runs[0], straight)
    assert any(v > 1e-12 for v in err.values()), err           # NOT the bitwise continuation ...
    assert err["rho"] < 1e-6 and err["c"] < 1e-2 and err["phi"] < 1e-2 and err["u"] < 0.3, err  # ... the same flow, re-started (u: 3e-2 here)


@pytest.mark.parametrize("save_mode,load_mode", [(0, 0), (0, 1), (1, 0)])
def test_checkpoint_continues_the_run_bit_for_bit(pkg, O, tmp_path, save_mode, load_mode):
    """ekpnp_save_checkpoint / ekpnp_load_checkpoint carry the post-collision populations too, so
    - unlike the reference's restart from fields - the reloaded run IS the interrupted one, bit for
    bit, whether the saving / loading context keeps two population buffers or one (in place), and
    at an odd or even step."""
    shape = (70, 5, 72)
    po = O.default_params(*shape)
    po.pb_iterations = 8
    p = pkg.default_params(*shape)
    p.pb_iterations = 8
    p.in_place = save_mode
    path = str(tmp_path / "ck.bin")
    with pkg.Solver(p) as s:
        s.initialization()
        s.set_fields(O.perturb_fields(po, s.fields()))
        s.fast_Poisson(); s.init_equilibrium(); s.step(7)
        s.save_checkpoint(path)
        s.step(6)
        want, t_want = s.fields(), s.t
    q = pkg.default_params(*shape)
    q.in_place = load_mode
    with pkg.Solver(q) as s:
        t = s.load_checkpoint(path)
        assert abs(t - 7 * p.dt) < 1e-22
        s.step(6)
        got = s.fields()
        assert abs(s.t - t_want) < 1e-22
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # a checkpoint taken right after init_equilibrium (no collide yet) continues as well
    with pkg.Solver(p) as s:
        s.initialization(); s.init_equilibrium()
        s.save_checkpoint(path)
        s.step(3)
        want = s.fields()
    with pkg.Solver(q) as s:
        s.load_checkpoint(path); s.step(3)
        got = s.fields()
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    wrong = pkg.default_params(shape[0], shape[1], shape[2] + 2)
    with pkg.Solver(wrong) as s, pytest.raises(pkg.EkpnpError, match="different lattice"):
        s.load_checkpoint(path)
