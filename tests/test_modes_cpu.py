"""CPU-side checks of the projection onto chosen x-y modes (include/ekpnp.h: ekpnp_modes_spec_check, ekpnp_mode_amplitudes,
ekpnp_modes_* and the ekpnp_group_* spellings; `ekpnp_main --modes-every`): declared, exported, mirrored in Python, bad specs
refused with a status and a message that names the offending number, NULL arguments refused.  No device needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1  # EKPNP_ERR_INVALID
W = (70, 66, 13)
VERBS = ["arm", "disarm", "record", "count", "read", "save"]
ENTRY_POINTS = (["ekpnp_modes_spec_check", "ekpnp_mode_amplitudes", "ekpnp_group_mode_amplitudes"] + ["ekpnp_modes_" + v for v in VERBS] +
                ["ekpnp_group_modes_" + v for v in VERBS])


def _header_code():
    txt = open(os.path.join(ROOT, "include", "ekpnp.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only, comments stripped


def test_the_entry_points_are_declared_exported_and_mirrored(pkg):
    assert len(ENTRY_POINTS) == 15
    code = _header_code()
    lib = pkg.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"include/ekpnp.h does not declare {name}"
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert name in pkg.exported_symbols()
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    assert re.search(r"#define\s+EKPNP_MAX_MODES\s+16\b", code) and pkg.MAX_MODES == 16
    assert re.search(r"typedef\s+struct\s+ekpnp_modes_spec\s*\{\s*int32_t\s+field_id;\s*int32_t\s+nmodes;\s*int32_t\s+m\[EKPNP_MAX_MODES\];\s*"
                     r"int32_t\s+n\[EKPNP_MAX_MODES\];\s*\}\s*ekpnp_modes_spec;", code)
    assert C.sizeof(pkg.ModesSpec) == 8 + 2 * 16 * 4 and [n for n, _ in pkg.ModesSpec._fields_] == ["field_id", "nmodes", "m", "n"]
    for cls in (pkg.Solver, pkg.Group):
        assert hasattr(cls, "mode_amplitudes"), cls.__name__
        for verb in VERBS:
            assert hasattr(cls, "modes_" + verb), (cls.__name__, verb)
    s = pkg.modes_spec("phi", [(0, 0), (3, -2), (35, 33)])
    assert (s.field_id, s.nmodes, list(s.m)[:3], list(s.n)[:3]) == (3, 3, [0, 3, 35], [0, -2, 33])


@pytest.mark.parametrize("field, modes, number", [
    (11, [(0, 0)], "11"),
    (-1, [(0, 0)], "-1"),
    ("uz", [], "0"),                               # nmodes 1 .. 16
    ("uz", [(0, 0)] * 17, "17"),
    ("uz", [(0, 0), (36, 0)], "36"),               # m outside 0 .. nx/2 = 35
    ("uz", [(-2, 0)], "-2"),
    ("uz", [(1, 34)], "34"),                       # n outside -(ny-1)/2 = -32 .. ny/2 = 33
    ("uz", [(1, 1), (1, -33)], "-33"),
])
def test_bad_specs_are_refused_with_the_offending_number(pkg, field, modes, number):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    spec = pkg.modes_spec(field, modes)
    assert lib.ekpnp_modes_spec_check(C.byref(p), C.byref(spec)) == INVALID
    msg = lib.ekpnp_last_error(None).decode()
    assert number in msg, msg
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.modes_spec_check(p, spec)
    assert "status 1" in str(e.value) and number in str(e.value), str(e.value)


def test_good_specs_are_accepted(pkg):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    for field in pkg.FIELDS:
        spec = pkg.modes_spec(field, [(0, 0), (1, 0), (0, 1), (35, 0), (3, -2), (35, 33), (1, 33), (17, -32)])
        assert lib.ekpnp_modes_spec_check(C.byref(p), C.byref(spec)) == 0, lib.ekpnp_last_error(None)
    assert lib.ekpnp_modes_spec_check(C.byref(p), C.byref(pkg.modes_spec("uz", [(k, k - 8) for k in range(16)]))) == 0
    q = pkg.default_params(9, 7, 5)  # odd extents: m <= 4, -3 <= n <= 3
    assert lib.ekpnp_modes_spec_check(C.byref(q), C.byref(pkg.modes_spec("c", [(4, -3), (4, 3)]))) == 0
    assert lib.ekpnp_modes_spec_check(C.byref(q), C.byref(pkg.modes_spec("c", [(4, 4)]))) == INVALID


def test_null_arguments_are_refused_not_dereferenced(pkg):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    spec = pkg.modes_spec("uz", [(1, 1)])
    buf = np.zeros(64)
    ptr = buf.ctypes.data_as(C.c_void_p)
    a, b = C.c_int64(), C.c_int64()
    assert lib.ekpnp_modes_spec_check(None, C.byref(spec)) == INVALID
    assert lib.ekpnp_modes_spec_check(C.byref(p), None) == INVALID
    for prefix in ("ekpnp_", "ekpnp_group_"):
        assert getattr(lib, prefix + "mode_amplitudes")(None, C.byref(spec), ptr) == INVALID
        assert getattr(lib, prefix + "modes_arm")(None, C.byref(spec), 4) == INVALID
        assert getattr(lib, prefix + "modes_disarm")(None) == INVALID
        assert getattr(lib, prefix + "modes_record")(None, 1, 0.0) == INVALID
        assert getattr(lib, prefix + "modes_count")(None, C.byref(a), C.byref(b)) == INVALID
        assert getattr(lib, prefix + "modes_read")(None, 0, 1, None, None, ptr) == INVALID
        assert getattr(lib, prefix + "modes_save")(None, b"/nonexistent/modes.dat") == INVALID
    assert (buf == 0.0).all()
