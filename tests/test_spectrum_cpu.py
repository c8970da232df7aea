"""CPU-side checks of the x-y power spectra (include/ekpnp.h: ekpnp_spectrum_spec_check, ekpnp_spectrum_shell_count,
ekpnp_spectrum_shells, ekpnp_spectrum_plane, ekpnp_spectrum, ekpnp_spectrum_* and the ekpnp_group_* spellings; `ekpnp_main
--spectrum-every`): declared, exported, mirrored in Python, bad specs refused with a status and a message that names the offending
number, the shell table equal to a Python transcription of its definition, NULL arguments refused.  No device needed."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1  # EKPNP_ERR_INVALID
W = (70, 66, 13)
VERBS = ["arm", "disarm", "record", "count", "read", "save"]
HOST_ONLY = ["ekpnp_spectrum_spec_check", "ekpnp_spectrum_shell_count", "ekpnp_spectrum_shells"]
ENTRY_POINTS = (HOST_ONLY + ["ekpnp_spectrum_plane", "ekpnp_spectrum", "ekpnp_group_spectrum_plane", "ekpnp_group_spectrum"] +
                ["ekpnp_spectrum_" + v for v in VERBS] + ["ekpnp_group_spectrum_" + v for v in VERBS])


def _header():
    return open(os.path.join(ROOT, "include", "ekpnp.h")).read()


def _header_code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)  # declarations only, comments stripped


def test_the_entry_points_are_declared_exported_and_mirrored(pkg):
    assert len(ENTRY_POINTS) == 19
    code = _header_code()
    lib = pkg.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"include/ekpnp.h does not declare {name}"
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert name in pkg.exported_symbols()
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    assert re.search(r"#define\s+EKPNP_MAX_SPECTRUM_PLANES\s+16\b", code) and pkg.MAX_SPECTRUM_PLANES == 16
    assert re.search(r"typedef\s+struct\s+ekpnp_spectrum_spec\s*\{\s*int32_t\s+field_id;\s*int32_t\s+nplanes;\s*"
                     r"int32_t\s+z\[EKPNP_MAX_SPECTRUM_PLANES\];\s*\}\s*ekpnp_spectrum_spec;", code)
    assert C.sizeof(pkg.SpectrumSpec) == 8 + 16 * 4 and [n for n, _ in pkg.SpectrumSpec._fields_] == ["field_id", "nplanes", "z"]
    for cls in (pkg.Solver, pkg.Group):
        for name in ["spectrum_shells", "spectrum_plane", "spectrum"] + ["spectrum_" + v for v in VERBS]:
            assert hasattr(cls, name), (cls.__name__, name)
    s = pkg.spectrum_spec("phi", [0, 3, 12])
    assert (s.field_id, s.nplanes, list(s.z)[:3]) == (3, 3, [0, 3, 12])
    assert pkg.spectrum_spec("uz").nplanes == 0


def test_the_file_header_is_documented():
    text = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())
    assert "# ekpnp spectrum nx <nx> ny <ny> nz <nz> field <name> planes <z ...> nshell <S> L <%.17g> recorded <r> dropped <d>" in text
    assert "# step time z peak_m peak_n peak_P E_0 ... E_<S-1>" in text
    main = open(os.path.join(ROOT, "ek-pnp-3d_amd", "csrc", "ekpnp_main.cpp")).read()
    for flag in ("--spectrum-every", "--spectrum-field", "--spectrum-planes"):
        assert flag in main, flag


@pytest.mark.parametrize("field, planes, nplanes, number", [
    (11, [0], None, "11"),
    (-1, [0], None, "-1"),
    ("uz", [], 17, "17"),                  # nplanes 0 .. 16
    ("uz", [], -1, "-1"),
    ("uz", [0, 13], None, "13"),           # z outside 0 .. nz - 1 = 12
    ("uz", [-2, 3], None, "-2"),
    ("uz", [1, 5, 5], None, "5"),          # strictly ascending
    ("uz", [1, 7, 4], None, "4"),
])
def test_bad_specs_are_refused_with_the_offending_number(pkg, field, planes, nplanes, number):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    spec = pkg.spectrum_spec(field, planes)
    if nplanes is not None:
        spec.nplanes = nplanes
    assert lib.ekpnp_spectrum_spec_check(C.byref(p), C.byref(spec)) == INVALID
    msg = lib.ekpnp_last_error(None).decode()
    assert number in msg, msg
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.spectrum_spec_check(p, spec)
    assert "status 1" in str(e.value) and number in str(e.value), str(e.value)


def test_good_specs_are_accepted(pkg):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    for field in pkg.FIELDS:
        for planes in (None, [0], [12], [0, 6, 12], list(range(13))):
            spec = pkg.spectrum_spec(field, planes)
            assert lib.ekpnp_spectrum_spec_check(C.byref(p), C.byref(spec)) == 0, lib.ekpnp_last_error(None)
    q = pkg.default_params(40, 12, 33)
    assert lib.ekpnp_spectrum_spec_check(C.byref(q), C.byref(pkg.spectrum_spec("c", list(range(1, 32, 2))))) == 0  # sixteen


def _shells_by_definition(p):
    """the definition of include/ekpnp.h transcribed: Python floats round every operation once"""
    nx, ny = p.nx, p.ny
    nxh = nx // 2 + 1
    L = max(p.Lx, p.Ly)
    rx = L / p.Lx
    ry = L / p.Ly
    out = np.zeros((ny, nxh), dtype=np.int64)
    ties = 0
    for n in range(ny):
        ns = n - ny if n > ny // 2 else n
        for m in range(nxh):
            a = float(m) * rx
            b = float(ns) * ry
            k2 = a * a + b * b
            r = math.sqrt(k2)
            out[n, m] = int(math.floor(r + 0.5))
            if r - math.floor(r) == 0.5:
                ties += 1
                assert out[n, m] == math.floor(r) + 1  # a tie goes up
    return out, ties


@pytest.mark.parametrize("nx, ny", [(40, 12), (70, 66), (64, 64), (50, 8)])
def test_the_shell_table_is_its_definition(pkg, nx, ny):
    lib = pkg.load_library()
    p = pkg.default_params(nx, ny, 17)
    want, ties = _shells_by_definition(p)
    if (nx, ny) == (50, 8):
        assert ties > 0 and p.Lx / p.Ly == 6.25  # n*ry = 12.5 exactly at m = 0, n = 2
    shell_of, count = pkg.spectrum_shells(p)
    n = C.c_int()
    assert lib.ekpnp_spectrum_shell_count(C.byref(p), C.byref(n)) == 0
    assert shell_of.shape == (ny, nx // 2 + 1) and shell_of.dtype == np.int32
    assert np.array_equal(shell_of, want)
    assert n.value == 1 + want.max() == len(count)
    assert count.sum() == ny * (nx // 2 + 1)
    assert np.array_equal(count, np.bincount(want.ravel(), minlength=n.value))
    assert shell_of[0, 0] == 0 and count[0] >= 1
    # count may be NULL
    again = np.zeros_like(shell_of)
    assert lib.ekpnp_spectrum_shells(C.byref(p), again.ctypes.data_as(C.c_void_p), None) == 0 and np.array_equal(again, shell_of)


def test_null_arguments_are_refused_not_dereferenced(pkg):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    spec = pkg.spectrum_spec("uz", [1])
    buf = np.zeros(64)
    ptr = buf.ctypes.data_as(C.c_void_p)
    a, b, n = C.c_int64(), C.c_int64(), C.c_int()
    assert lib.ekpnp_spectrum_spec_check(None, C.byref(spec)) == INVALID
    assert lib.ekpnp_spectrum_spec_check(C.byref(p), None) == INVALID
    assert lib.ekpnp_spectrum_shell_count(None, C.byref(n)) == INVALID
    assert lib.ekpnp_spectrum_shell_count(C.byref(p), None) == INVALID
    assert lib.ekpnp_spectrum_shells(None, ptr, None) == INVALID
    assert lib.ekpnp_spectrum_shells(C.byref(p), None, None) == INVALID
    for prefix in ("ekpnp_", "ekpnp_group_"):
        assert getattr(lib, prefix + "spectrum_plane")(None, 6, 1, ptr) == INVALID
        assert getattr(lib, prefix + "spectrum")(None, C.byref(spec), ptr, ptr) == INVALID
        assert getattr(lib, prefix + "spectrum_arm")(None, C.byref(spec), 4) == INVALID
        assert getattr(lib, prefix + "spectrum_disarm")(None) == INVALID
        assert getattr(lib, prefix + "spectrum_record")(None, 1, 0.0) == INVALID
        assert getattr(lib, prefix + "spectrum_count")(None, C.byref(a), C.byref(b)) == INVALID
        assert getattr(lib, prefix + "spectrum_read")(None, 0, 1, None, None, ptr, ptr) == INVALID
        assert getattr(lib, prefix + "spectrum_save")(None, b"/nonexistent/spectrum.dat") == INVALID
    assert (buf == 0.0).all()
