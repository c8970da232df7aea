"""CPU tests of the tracers' sort by cell (csrc/tracers.hip; include/ekpnp.h: ekpnp_tracers_sort_key, ekpnp_tracers_sort_host): the
host-only entry points, which ARE the definition the device sort is held against in tests/test_tracers_sort_gpu.py.  No device
is needed.  The key is integer arithmetic and the stable order of the keys is unique, so every comparison is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _tracers_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
SHAPES = {"W": (70, 66, 13), "O": (35, 33, 5), "R": (40, 12, 17)}
LOST = 0xFFFFFFFF


def keys_ref(shape, x, y, z):
    """the header's text in numpy: (k0*ny + j0)*nx + i0 with the stencil's indices, 0xFFFFFFFF for a lost particle"""
    nx, ny, nz = shape
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    lost = np.isnan(x) | np.isnan(y) | np.isnan(z)
    xs, ys, zs = (np.where(lost, 0.0, a) for a in (x, y, z))
    i0, j0, k0 = xs.astype(np.int64), ys.astype(np.int64), np.minimum(zs.astype(np.int64), nz - 2)
    return np.where(lost, LOST, (k0 * ny + j0) * nx + i0).astype(np.uint32)


def _lattice(pkg, nx, ny, nz):
    """parameters of a lattice ekpnp_default_params itself would not make (it wants nz >= 4)"""
    p = pkg.default_params(nx, ny, max(nz, 4))
    p.nz = nz
    return p


def test_entry_points_are_declared_exported_and_mirrored(pkg):
    lib = pkg.load_library()
    for name in ("ekpnp_tracers_sort_key", "ekpnp_tracers_sort_host", "ekpnp_tracers_sort", "ekpnp_tracers_ids"):
        assert name in pkg.exported_symbols()
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    assert lib.ekpnp_tracers_sort_key.restype is C.c_uint32
    assert not [n for n in pkg.exported_symbols() if n.startswith("ekpnp_group_tracers")]
    for m in ("tracers_sort", "tracers_ids", "tracers_get"):
        assert hasattr(pkg.Solver, m), m
    assert callable(pkg.tracers_sort_key) and callable(pkg.tracers_sort_host) and pkg.TRACERS_KEY_LOST == LOST
    assert not [m for m in dir(pkg.Group) if "tracers" in m]


@pytest.mark.parametrize("shape", ["W", "O", "R"])
def test_key_equals_the_transcription(pkg, shape):
    s = SHAPES[shape]
    nx, ny, nz = s
    p = pkg.default_params(*s)
    x, y, z = T.special_cloud(s, 1000, 17)
    got = pkg.tracers_sort_key(p, x, y, z)
    assert got.dtype == np.uint32 and np.array_equal(got, keys_ref(s, x, y, z))
    # the special ones: z = nz-1 clamps to the plane nz-2, y one ulp below ny is row ny-1, the lost one
    assert got[4] == ((nz - 2) * ny + 5) * nx + 6 and got[5] == ((nz - 2) * ny + 6) * nx + 7
    assert got[2] == (2 * ny + ny - 1) * nx + 3 and got[1] == (2 * ny + 1) * nx + nx - 1 and got[12] == LOST
    assert got[:12].max() < nx * ny * (nz - 1)
    # x just below nx, the last node of the last key plane, the first node; NaN in one coordinate alone loses the particle
    edge = pkg.tracers_sort_key(p, [np.nextafter(float(nx), 0.0), 0.0, 1.0, 1.0, np.nan], [np.nextafter(float(ny), 0.0), 0.0, np.nan, 1.0, 1.0],
                                [float(nz - 1), 0.0, 1.0, np.nan, 1.0])
    assert edge.tolist() == [nx * ny * (nz - 1) - 1, 0, LOST, LOST, LOST]


@pytest.mark.parametrize("n", [0, 1, 1000, 4097])
def test_sort_host_is_the_stable_argsort_of_the_keys(pkg, n):
    for s in SHAPES.values():
        p = pkg.default_params(*s)
        x, y, z = T.special_cloud(s, n, 23 + n) if n else (np.zeros(0),) * 3
        if n >= 1000:   # many equal keys, and more lost ones in the middle
            x[200:400], y[200:400], z[200:400] = x[150], y[150], z[150]
            x[500:520] = np.nan
        perm = pkg.tracers_sort_host(p, x, y, z)
        keys = keys_ref(s, x, y, z)
        assert perm.dtype == np.int32 and np.array_equal(perm, np.argsort(keys, kind="stable"))
        if n >= 1000:
            lost = np.flatnonzero(keys == LOST)
            assert lost.size >= 21 and np.array_equal(perm[n - lost.size:], lost)   # at the end, in their slot order


def test_one_key_for_all_and_an_all_lost_cloud_give_the_identity(pkg):
    p = pkg.default_params(*SHAPES["W"])
    rng = np.random.default_rng(3)
    for n in (1, 1000, 4097):
        x, y, z = 20.0 + rng.uniform(0, 1, n), 30.0 + rng.uniform(0, 1, n), 6.0 + rng.uniform(0, 1, n)
        assert np.array_equal(pkg.tracers_sort_host(p, x, y, z), np.arange(n))
        nan = np.full(n, np.nan)
        assert np.array_equal(pkg.tracers_sort_host(p, nan, nan, nan), np.arange(n))
    # reversed memory order: the perm is the reversal
    k = np.arange(999, -1, -1)
    x, y, z = (k % 70) + 0.5, ((k // 70) % 66) + 0.5, (k // 4620) + 0.5
    assert np.array_equal(pkg.tracers_sort_host(p, x, y, z), k)


def test_refusals_name_the_offending_number(pkg):
    L = pkg.load_library()
    p = pkg.default_params(*SHAPES["W"])
    a = np.zeros(10)
    perm = np.zeros(10, dtype=np.int32)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    err = lambda: L.ekpnp_last_error(None).decode()
    assert L.ekpnp_tracers_sort_host(C.byref(p), 10, ptr(a), ptr(a), ptr(a), ptr(perm)) == 0
    assert L.ekpnp_tracers_sort_host(None, 10, ptr(a), ptr(a), ptr(a), ptr(perm)) == 1 and "NULL" in err()
    for k in range(4):
        args = [ptr(a), ptr(a), ptr(a), ptr(perm)]
        args[k] = None
        assert L.ekpnp_tracers_sort_host(C.byref(p), 10, *args) == 1 and "NULL" in err(), k
    assert L.ekpnp_tracers_sort_key(None, 1.0, 1.0, 1.0) == LOST and "NULL" in err()
    assert L.ekpnp_tracers_sort_host(C.byref(p), -1, ptr(a), ptr(a), ptr(a), ptr(perm)) == 1 and "n = -1" in err()
    assert L.ekpnp_tracers_sort_host(C.byref(p), (1 << 28) + 1, ptr(a), ptr(a), ptr(a), ptr(perm)) == 1 and "n = 268435457" in err()
    flat = _lattice(pkg, 70, 66, 2)
    assert L.ekpnp_tracers_sort_host(C.byref(flat), 10, ptr(a), ptr(a), ptr(a), ptr(perm)) == 1 and "nz = 2" in err()
    assert L.ekpnp_tracers_sort_key(C.byref(flat), 1.0, 1.0, 1.0) == LOST and "nz = 2" in err()
    # 65536 x 65536 x 3: nx*ny*(nz-1) = 2^33
    huge = _lattice(pkg, 65536, 65536, 3)
    assert L.ekpnp_tracers_sort_host(C.byref(huge), 10, ptr(a), ptr(a), ptr(a), ptr(perm)) == 1 and "nx*ny*(nz-1) = 8589934592" in err()
    assert L.ekpnp_tracers_sort_key(C.byref(huge), 1.0, 1.0, 1.0) == LOST and "8589934592" in err()
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.tracers_sort_host(huge, a, a, a)
    assert "8589934592" in str(e.value) and "status 1" in str(e.value)
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.tracers_sort_key(huge, a, a, a)
    assert "8589934592" in str(e.value)
    # exactly at the limit: 2^32 - 1 = 3 * 21845 * 65537 is the first product refused (its largest key would be the lost particles');
    # one row less per plane is taken, and its last node has the largest key there is
    first = pkg.default_params(21845, 65537, 4)
    assert L.ekpnp_tracers_sort_key(C.byref(first), 1.0, 1.0, 1.0) == LOST and "4294967295" in err()
    last = pkg.default_params(21845, 65536, 4)
    assert pkg.tracers_sort_key(last, [21844.5, 0.0], [65535.5, 0.0], [3.0, 0.0]).tolist() == [21845 * 65536 * 3 - 1, 0]


def test_driver_refuses_a_sort_without_a_cloud_and_k_below_one():
    assert os.path.exists(EXE), "ekpnp_main not built"
    geo = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "2"]
    for args, msg in ((["--tracers", "10", "--tracers-sort-every", "0"], "got 0"), (["--tracers", "10", "--tracers-sort-every", "-3"], "got -3"),
                      (["--tracers-sort-every", "3"], "no cloud to sort")):
        r = subprocess.run([EXE, *geo, *args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--tracers-sort-every" in r.stderr and msg in r.stderr, (args, r.returncode, r.stderr[-500:])
    r = subprocess.run([EXE, "--help-me"], capture_output=True, text=True, timeout=120)
    assert "--tracers-sort-every K" in r.stderr
