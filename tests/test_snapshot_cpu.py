"""CPU-side checks of the coarsened FP32 snapshots (include/ekpnp.h: ekpnp_snapshot_extent / _read / _begin / _finish /
_pending and their ekpnp_group_* spellings): declared, exported, mirrored in Python, the extent arithmetic, and bad
arguments refused with a status and a message that names the offending number.  No device needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = [
    "ekpnp_snapshot_extent", "ekpnp_snapshot_read", "ekpnp_snapshot_begin", "ekpnp_snapshot_finish", "ekpnp_snapshot_pending",
    "ekpnp_group_snapshot_read", "ekpnp_group_snapshot_begin", "ekpnp_group_snapshot_finish", "ekpnp_group_snapshot_pending",
]
INVALID = 1  # EKPNP_ERR_INVALID


def _header_code():
    txt = open(os.path.join(ROOT, "include", "ekpnp.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only, comments stripped


def test_the_entry_points_are_declared_exported_and_mirrored(pkg):
    code = _header_code()
    lib = pkg.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"include/ekpnp.h does not declare {name}"
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert name in pkg.exported_symbols()
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    m = re.search(r"typedef\s+struct\s+ekpnp_snapshot_spec\s*\{\s*uint32_t\s+fields;\s*int32_t\s+cx,\s*cy,\s*cz;\s*\}\s*ekpnp_snapshot_spec;", code)
    assert m, "ekpnp_snapshot_spec is not {uint32_t fields; int32_t cx, cy, cz;}"
    assert C.sizeof(pkg.SnapshotSpec) == 16 and [n for n, _ in pkg.SnapshotSpec._fields_] == ["fields", "cx", "cy", "cz"]
    for cls in (pkg.Solver, pkg.Group):
        for method in ("snapshot", "snapshot_begin", "snapshot_finish", "snapshot_pending"):
            assert hasattr(cls, method), (cls.__name__, method)
    assert callable(pkg.snapshot_extent)


def test_extent_arithmetic(pkg):
    p = pkg.default_params(512, 512, 513)
    assert pkg.snapshot_extent(p, None, (2, 2, 2)) == (256, 256, 257, 11 * 256 * 256 * 257 * 4)
    assert pkg.snapshot_extent(p, ["uz", "c", "cn"], (8, 4, 512)) == (64, 128, 2, 3 * 64 * 128 * 2 * 4)
    assert pkg.snapshot_extent(p, 1 << 10, (1, 1, 1)) == (512, 512, 513, 512 * 512 * 513 * 4)
    # any of the out pointers may be NULL
    lib = pkg.load_library()
    spec = pkg.snapshot_spec(None, (2, 2, 2))
    z = C.c_int()
    assert lib.ekpnp_snapshot_extent(C.byref(p), C.byref(spec), None, None, C.byref(z), None) == 0 and z.value == 257


@pytest.mark.parametrize("shape, fields, coarsen, number", [
    ((48, 8, 9), None, (3, 1, 1), "3"),          # cx is not 1, 2, 4 or 8
    ((48, 8, 9), None, (1, 16, 1), "16"),        # nor is cy
    ((50, 8, 9), None, (4, 1, 1), "50"),         # cx = 4 does not divide nx = 50
    ((48, 12, 9), None, (1, 8, 1), "12"),        # cy = 8 does not divide ny = 12
    ((48, 8, 51), None, (1, 1, 4), "50"),        # cz = 4 does not divide nz - 1 = 50
    ((48, 8, 9), None, (1, 1, 0), "0"),          # cz >= 1
    ((48, 8, 9), 1 << 11, (1, 1, 1), "2048"),    # a bit above field 10
])
def test_bad_specs_are_refused_with_the_offending_number(pkg, shape, fields, coarsen, number):
    p = pkg.default_params(*shape)
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.snapshot_extent(p, fields, coarsen)
    assert "status 1" in str(e.value) and number in str(e.value), str(e.value)


def test_null_arguments_are_refused_not_dereferenced(pkg):
    lib = pkg.load_library()
    p = pkg.default_params(48, 8, 9)
    spec = pkg.snapshot_spec(None, (2, 2, 2))
    buf = (C.c_float * 16)()
    a, b = C.c_int(), C.c_int()
    assert lib.ekpnp_snapshot_extent(None, C.byref(spec), None, None, None, None) == INVALID
    assert lib.ekpnp_snapshot_extent(C.byref(p), None, None, None, None, None) == INVALID
    assert lib.ekpnp_snapshot_read(None, C.byref(spec), buf, C.byref(a), C.byref(b)) == INVALID
    assert lib.ekpnp_snapshot_begin(None, C.byref(spec), b"/nonexistent/x.vtk", 0.0) == INVALID
    assert lib.ekpnp_snapshot_finish(None) == INVALID
    assert lib.ekpnp_snapshot_pending(None) == 0
    assert lib.ekpnp_group_snapshot_read(None, C.byref(spec), buf) == INVALID
    assert lib.ekpnp_group_snapshot_begin(None, C.byref(spec), b"/nonexistent/x.vtk", 0.0) == INVALID
    assert lib.ekpnp_group_snapshot_finish(None) == INVALID
    assert lib.ekpnp_group_snapshot_pending(None) == 0


@pytest.mark.parametrize("flag", ["--snap-every", "--snap-coarsen", "--snap-fields"])
def test_driver_flag_without_a_value_prints_the_usage(pkg, flag):
    exe = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
    assert os.path.exists(exe), "ekpnp_main not built"
    r = subprocess.run([exe, flag], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "usage: ekpnp_main" in r.stderr and "--snap-every N" in r.stderr and "--snap-coarsen cx,cy,cz" in r.stderr
    assert "--snap-fields rho,uz,..." in r.stderr and "snap_<step, 7 digits>.vtk" in r.stderr
