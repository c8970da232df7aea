"""CPU-side checks of the sections (include/ekpnp.h: ekpnp_section_sum, ekpnp_section_spec_check, ekpnp_section_extent, ekpnp_section,
ekpnp_section_save, ekpnp_section_* and the ekpnp_group_* spellings; `ekpnp_main --section-every / --section-full-every`): declared,
exported, mirrored in Python, the file headers documented, bad specs refused with a status and a message that names the offending
number, NULL arguments refused, the extents right, and the sum equal to a numpy transcription of its definition, addition by
addition.  No device needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1  # EKPNP_ERR_INVALID
W = (70, 66, 13)
VERBS = ["arm", "disarm", "record", "count", "read", "ring_save"]
HOST_ONLY = ["ekpnp_section_sum", "ekpnp_section_spec_check", "ekpnp_section_extent"]
ENTRY_POINTS = (HOST_ONLY + ["ekpnp_section", "ekpnp_section_save", "ekpnp_group_section", "ekpnp_group_section_save"] +
                ["ekpnp_section_" + v for v in VERBS] + ["ekpnp_group_section_" + v for v in VERBS])


def _header():
    return open(os.path.join(ROOT, "include", "ekpnp.h")).read()


def _header_code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)  # declarations only, comments stripped


def test_the_entry_points_are_declared_exported_and_mirrored(pkg):
    assert len(ENTRY_POINTS) == 19
    code = _header_code()
    lib = pkg.load_library()
    for name in ENTRY_POINTS:
        kind = "double" if name == "ekpnp_section_sum" else "int"
        assert re.search(r"\b%s\s+%s\s*\(" % (kind, name), code), f"include/ekpnp.h does not declare {name}"
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert name in pkg.exported_symbols()
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    assert lib.ekpnp_section_sum.restype is C.c_double
    assert re.search(r"#define\s+EKPNP_SECTION_Q\s+11\b", code) and pkg.SECTION_Q == 11 and pkg.SECTION_VALUES == pkg.FIELDS + ["q"]
    assert re.search(r"#define\s+EKPNP_ACROSS_X\s+0\b", code) and re.search(r"#define\s+EKPNP_ACROSS_Y\s+1\b", code)
    assert (pkg.ACROSS_X, pkg.ACROSS_Y) == (0, 1)
    assert re.search(r"#define\s+EKPNP_MAX_SECTION_PLANES\s+16\b", code) and pkg.MAX_SECTION_PLANES == 16
    assert re.search(r"typedef\s+struct\s+ekpnp_section_spec\s*\{\s*uint32_t\s+values;\s*int32_t\s+across,\s*lo,\s*hi,\s*nplanes;\s*"
                     r"int32_t\s+z\[EKPNP_MAX_SECTION_PLANES\];\s*\}\s*ekpnp_section_spec;", code)
    assert C.sizeof(pkg.SectionSpec) == 4 * 5 + 4 * 16
    assert [n for n, _ in pkg.SectionSpec._fields_] == ["values", "across", "lo", "hi", "nplanes", "z"]
    for cls in (pkg.Solver, pkg.Group):
        for name in ["section", "section_write"] + ["section_" + v for v in ("arm", "disarm", "record", "count", "read", "save")]:
            assert hasattr(cls, name), (cls.__name__, name)
    s = pkg.section_spec(["uz", "q"], "y", (3, 67), planes=[0, 5, 12])
    assert (s.values, s.across, s.lo, s.hi, s.nplanes, list(s.z[:3])) == ((1 << 6) | (1 << 11), 1, 3, 67, 3, [0, 5, 12])
    assert s.names == ["uz", "q"]
    s = pkg.section_spec(None, "x", None, n=70)
    assert (s.values, s.across, s.lo, s.hi, s.nplanes) == (0, 0, 0, 69, 0) and s.names == pkg.SECTION_VALUES


def test_the_file_headers_are_documented():
    text = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())
    assert ("# ekpnp section nx <nx> ny <ny> nz <nz> across <x|y> lo <lo> hi <hi> values <names...> nkeep <n> time <%.17g>") in text
    assert "name z v_0 ... v_<nkeep-1>" in text
    assert "planes <z ...> recorded <r> dropped <d>" in text
    assert "step time name z v_0 ... v_<nkeep-1>" in text
    assert "rho c cn phi ux uy uz Ex Ey Ez T q" in text
    main = open(os.path.join(ROOT, "ek-pnp-3d_amd", "csrc", "ekpnp_main.cpp")).read()
    for flag in ("--section-every", "--section-full-every", "--section-values", "--section-across", "--section-range", "--section-planes"):
        assert flag in main, flag


def _spec(pkg, values=("uz",), across=0, lo=0, hi=5, planes=None):
    return pkg.section_spec(values, across, (lo, hi), planes)


@pytest.mark.parametrize("kw, number", [
    (dict(values=1 << 12), "4096"),                      # a bit above 11
    (dict(values=(1 << 6) | (1 << 20)), str((1 << 6) | (1 << 20))),
    (dict(across=2), "across = 2"),
    (dict(across=-1), "across = -1"),
    (dict(across=0, lo=0, hi=70), "hi = 70"),           # across x: < nx = 70
    (dict(across=1, lo=0, hi=66), "hi = 66"),           # across y: < ny = 66
    (dict(across=1, lo=66, hi=69), "lo = 66"),
    (dict(lo=-1, hi=5), "lo = -1"),
    (dict(lo=3, hi=-2), "hi = -2"),
    (dict(lo=9, hi=4), "lo = 9"),                        # lo > hi
    (dict(planes=list(range(17))), "nplanes = 17"),
    (dict(planes=[0, 13]), "z = 13"),                    # z < nz = 13
    (dict(planes=[-1, 3]), "z = -1"),
    (dict(planes=[2, 5, 5]), "z = 5"),                   # not strictly ascending
    (dict(planes=[7, 3]), "z = 3"),
])
def test_bad_specs_are_refused_with_the_offending_number(pkg, kw, number):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    spec = _spec(pkg, **kw)
    if kw.get("planes") and len(kw["planes"]) > 16:
        assert spec.nplanes == 17
    assert lib.ekpnp_section_spec_check(C.byref(p), C.byref(spec)) == INVALID
    msg = lib.ekpnp_last_error(None).decode()
    assert number in msg, msg
    nv, nk = C.c_int(-7), C.c_int(-7)
    assert lib.ekpnp_section_extent(C.byref(p), C.byref(spec), C.byref(nv), C.byref(nk)) == INVALID
    assert number in lib.ekpnp_last_error(None).decode() and (nv.value, nk.value) == (-7, -7)
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.section_spec_check(p, spec)
    assert "status 1" in str(e.value) and number in str(e.value), str(e.value)


def test_good_specs_are_accepted_and_the_extents_are_right(pkg):
    lib = pkg.load_library()
    nx, ny, nz = W
    p = pkg.default_params(*W)
    assert pkg.section_extent(p, pkg.section_spec(None, "x", (0, nx - 1))) == (12, ny)
    assert pkg.section_extent(p, pkg.section_spec(None, "y", (0, ny - 1))) == (12, nx)
    assert pkg.section_extent(p, pkg.section_spec((1 << 12) - 1, "y", (5, 5))) == (12, nx)
    assert pkg.section_extent(p, pkg.section_spec(["q"], "x", (69, 69), planes=[12])) == (1, ny)
    assert pkg.section_extent(p, pkg.section_spec(["c", "q", "rho"], 1, (3, 65), planes=list(range(13)))) == (3, nx)
    assert pkg.section_extent(p, pkg.section_spec(["phi", "Ez"], 0, (0, 0), planes=list(range(0, 13))[:16])) == (2, ny)
    for v in pkg.SECTION_VALUES:
        for across, n in ((0, nx), (1, ny)):
            for lo, hi in ((0, n - 1), (0, 0), (n - 1, n - 1), (3, n - 3)):
                spec = pkg.section_spec([v], across, (lo, hi), planes=[0, 5, nz - 1])
                assert lib.ekpnp_section_spec_check(C.byref(p), C.byref(spec)) == 0, lib.ekpnp_last_error(None)
    assert pkg.section_spec_check(p, pkg.section_spec(["uz"], "y", (1, 2))).hi == 2


def test_null_arguments_are_refused_not_dereferenced(pkg):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    spec = _spec(pkg)
    buf = np.zeros(64)
    ptr = buf.ctypes.data_as(C.c_void_p)
    a, b = C.c_int64(), C.c_int64()
    nv, nk = C.c_int(), C.c_int()
    assert lib.ekpnp_section_spec_check(None, C.byref(spec)) == INVALID
    assert lib.ekpnp_section_spec_check(C.byref(p), None) == INVALID
    assert lib.ekpnp_section_extent(None, C.byref(spec), C.byref(nv), C.byref(nk)) == INVALID
    assert lib.ekpnp_section_extent(C.byref(p), None, C.byref(nv), C.byref(nk)) == INVALID
    assert lib.ekpnp_section_extent(C.byref(p), C.byref(spec), None, C.byref(nk)) == INVALID
    assert lib.ekpnp_section_extent(C.byref(p), C.byref(spec), C.byref(nv), None) == INVALID
    for prefix in ("ekpnp_", "ekpnp_group_"):
        assert getattr(lib, prefix + "section")(None, C.byref(spec), ptr) == INVALID
        assert getattr(lib, prefix + "section_save")(None, C.byref(spec), b"/nonexistent/section.dat", 0.0) == INVALID
        assert getattr(lib, prefix + "section_arm")(None, C.byref(spec), 4) == INVALID
        assert getattr(lib, prefix + "section_disarm")(None) == INVALID
        assert getattr(lib, prefix + "section_record")(None, 1, 0.0) == INVALID
        assert getattr(lib, prefix + "section_count")(None, C.byref(a), C.byref(b)) == INVALID
        assert getattr(lib, prefix + "section_read")(None, 0, 1, None, None, ptr) == INVALID
        assert getattr(lib, prefix + "section_ring_save")(None, b"/nonexistent/section.dat") == INVALID
    assert (buf == 0.0).all()


def definition(v, stride, n):
    """include/ekpnp.h transcribed into numpy float64: runs of 64 consecutive indices from i = 0, each run added in ascending i
    starting from its first term, the run sums added in ascending run starting from the first"""
    t = np.asarray(v, dtype=np.float64)[::stride][:n]
    assert len(t) == n
    S = None
    with np.errstate(invalid="ignore", over="ignore"):
        for i0 in range(0, n, 64):
            r = t[i0]
            for x in t[i0 + 1:i0 + 64]:
                r = r + x
            S = r if S is None else S + r
    return np.float64(S)


def _bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize("stride", [1, 7])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 128, 129, 200])
def test_section_sum_is_its_definition(pkg, n, stride):
    rng = np.random.default_rng(100 * n + stride)
    for scale in (1.0, 1e-3):
        v = scale * rng.uniform(-1.0, 1.0, size=n * stride) * 10.0 ** rng.integers(-6, 6, size=n * stride)  # cancellation: the order shows
        got = pkg.section_sum(v, stride, n)
        assert _bits(got) == _bits(definition(v, stride, n)), (n, stride, got)
    if n >= 129 and stride == 1:
        # the order is THIS one: neither one left-to-right pass nor numpy's pairwise sum give the same bits for every such vector
        others = 0
        for k in range(20):
            v = rng.uniform(-1.0, 1.0, size=n)
            left = np.float64(0.0)
            for x in v:
                left = left + x
            others += _bits(pkg.section_sum(v)) != _bits(left)
            assert _bits(pkg.section_sum(v)) == _bits(definition(v, 1, n))
        assert others > 0


def test_section_sum_of_one_term_is_the_term_and_a_nan_stays_in_its_sum(pkg):
    for x in (-0.0, 0.0, 5e-324, -np.inf, 1.5):
        assert _bits(pkg.section_sum(np.array([x]), 1, 1)) == _bits(x)
        assert _bits(pkg.section_sum(np.array([x, 3.0, 4.0]), 3, 1)) == _bits(x)
    assert _bits(pkg.section_sum(np.array([-0.0, -0.0]))) == _bits(-0.0)   # no zero is padded in: (+0.0) + (-0.0) would be +0.0
    v = np.ones(200)
    for where in (0, 63, 64, 130, 199):
        w = v.copy()
        w[where] = np.nan
        assert np.isnan(pkg.section_sum(w))
    w = v.copy()
    w[70] = np.inf
    assert pkg.section_sum(w) == np.inf
    w[150] = -np.inf
    assert np.isnan(pkg.section_sum(w))
    assert pkg.section_sum(v) == 200.0
