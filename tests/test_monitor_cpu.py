"""CPU-side checks of the per-step scalar time series (include/ekpnp.h: ekpnp_monitor_* and the ekpnp_group_monitor_*
spellings): declared, exported, mirrored in Python, and bad specs refused with a status and a message that names the
offending number.  No device needed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VERBS = ["sample", "arm", "disarm", "record", "count", "read", "save"]
ENTRY_POINTS = (["ekpnp_monitor_name", "ekpnp_monitor_spec_check"] + ["ekpnp_monitor_" + v for v in VERBS] +
                ["ekpnp_group_monitor_" + v for v in VERBS])
NAMES = ["current_top", "current_bottom", "dTdz_bottom", "dTdz_top", "uz_max", "u_u", "q", "q_q", "uz_T", "rho_dev", "nonfinite"]
INVALID = 1  # EKPNP_ERR_INVALID


def _header_code():
    txt = open(os.path.join(ROOT, "include", "ekpnp.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only, comments stripped


def test_the_entry_points_are_declared_exported_and_mirrored(pkg):
    assert len(ENTRY_POINTS) == 16
    code = _header_code()
    lib = pkg.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|const\s+char\s*\*)\s*%s\s*\(" % name, code), f"include/ekpnp.h does not declare {name}"
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert name in pkg.exported_symbols()
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    m = re.search(r"typedef\s+struct\s+ekpnp_monitor_spec\s*\{\s*uint32_t\s+quantities;\s*int32_t\s+every;\s*int32_t\s+capacity;\s*\}\s*ekpnp_monitor_spec;", code)
    assert m, "ekpnp_monitor_spec is not {uint32_t quantities; int32_t every; int32_t capacity;}"
    assert C.sizeof(pkg.MonitorSpec) == 12 and [n for n, _ in pkg.MonitorSpec._fields_] == ["quantities", "every", "capacity"]
    assert re.search(r"\bEKPNP_NMONITORS\s*=\s*11\b", code)
    assert pkg.MONITOR_NAMES == NAMES and pkg.MONITOR_ID == {n: i for i, n in enumerate(NAMES)}
    for i, n in enumerate(NAMES):
        assert lib.ekpnp_monitor_name(i) == n.encode()
    assert lib.ekpnp_monitor_name(-1) is None and lib.ekpnp_monitor_name(11) is None
    for cls in (pkg.Solver, pkg.Group):
        for verb in VERBS:
            assert hasattr(cls, "monitor_" + verb), (cls.__name__, verb)


@pytest.mark.parametrize("quantities, every, capacity, number", [
    (0, 0, 8, "0"),            # every >= 1
    (0, 1, 0, "0"),            # capacity >= 1
    (0, 1, -3, "-3"),
    (1 << 11, 1, 8, "2048"),   # a bit above id 10
])
def test_bad_specs_are_refused_with_the_offending_number(pkg, quantities, every, capacity, number):
    lib = pkg.load_library()
    spec = pkg.MonitorSpec(quantities, every, capacity)
    assert lib.ekpnp_monitor_spec_check(C.byref(spec)) == INVALID
    msg = lib.ekpnp_last_error(None).decode()
    assert number in msg, msg
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.monitor_spec_check(quantities, every, capacity)
    assert "status 1" in str(e.value) and number in str(e.value), str(e.value)


def test_good_specs_are_accepted(pkg):
    lib = pkg.load_library()
    for spec in (pkg.MonitorSpec(0, 1, 1), pkg.MonitorSpec((1 << 11) - 1, 7, 1 << 20), pkg.MonitorSpec(1 << 10, 1, 64)):
        assert lib.ekpnp_monitor_spec_check(C.byref(spec)) == 0
    assert pkg.monitor_spec_check(["current_top", "uz_max"], 2, 5).quantities == 0b10001
    assert pkg.monitor_mask(None) == 0 and pkg.monitor_mask([10]) == 1 << 10


def test_null_arguments_are_refused_not_dereferenced(pkg):
    lib = pkg.load_library()
    spec = pkg.MonitorSpec(0, 1, 4)
    buf = (C.c_double * 11)()
    a, b = C.c_int64(), C.c_int64()
    assert lib.ekpnp_monitor_spec_check(None) == INVALID
    for prefix in ("ekpnp_monitor_", "ekpnp_group_monitor_"):
        assert getattr(lib, prefix + "sample")(None, 0, buf) == INVALID
        assert getattr(lib, prefix + "arm")(None, C.byref(spec)) == INVALID
        assert getattr(lib, prefix + "disarm")(None) == INVALID
        assert getattr(lib, prefix + "record")(None, 1, 0.0) == INVALID
        assert getattr(lib, prefix + "count")(None, C.byref(a), C.byref(b)) == INVALID
        assert getattr(lib, prefix + "read")(None, 0, 1, None, None, buf) == INVALID
        assert getattr(lib, prefix + "save")(None, b"/nonexistent/monitor.dat") == INVALID


@pytest.mark.parametrize("flag", ["--monitor-every", "--monitor-quantities"])
def test_driver_flag_without_a_value_prints_the_usage(pkg, flag):
    exe = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
    assert os.path.exists(exe), "ekpnp_main not built"
    r = subprocess.run([exe, flag], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "usage: ekpnp_main" in r.stderr and "--monitor-every N" in r.stderr and "monitor.dat" in r.stderr
    assert "--monitor-quantities current_top,uz_max,..." in r.stderr


def test_driver_refuses_an_unknown_quantity_by_name(pkg):
    exe = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
    r = subprocess.run([exe, "--monitor-quantities", "uz_max,vorticity"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "current_top,current_bottom" in r.stderr and "vorticity" in r.stderr
