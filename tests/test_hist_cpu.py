"""CPU-side checks of the histograms (include/ekpnp.h: ekpnp_hist_bin, ekpnp_hist_spec_check, ekpnp_hist_range_check,
ekpnp_hist_planes, ekpnp_value_range, ekpnp_hist_* and the ekpnp_group_* spellings; `ekpnp_main --hist-every`): declared, exported,
mirrored in Python, the file header documented, bad specs refused with a status and a message that names the offending number,
NULL arguments refused, and the index function equal to a numpy transcription of its definition, operation by operation.  No
device needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1  # EKPNP_ERR_INVALID
W = (70, 66, 13)
VERBS = ["arm", "disarm", "record", "count", "read", "save"]
HOST_ONLY = ["ekpnp_hist_bin", "ekpnp_hist_spec_check", "ekpnp_hist_range_check"]
ENTRY_POINTS = (HOST_ONLY + ["ekpnp_hist_planes", "ekpnp_value_range", "ekpnp_group_hist_planes", "ekpnp_group_value_range"] +
                ["ekpnp_hist_" + v for v in VERBS] + ["ekpnp_group_hist_" + v for v in VERBS])


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
    assert re.search(r"#define\s+EKPNP_HIST_Q\s+11\b", code) and pkg.HIST_Q == 11 and pkg.HIST_VALUES == pkg.FIELDS + ["q"]
    assert re.search(r"#define\s+EKPNP_HIST_MAX_BINS\s+4096\b", code) and pkg.HIST_MAX_BINS == 4096
    assert re.search(r"typedef\s+struct\s+ekpnp_hist_axis\s*\{\s*int32_t\s+value;\s*int32_t\s+n;\s*double\s+lo,\s*hi;\s*\}\s*ekpnp_hist_axis;", code)
    assert re.search(r"typedef\s+struct\s+ekpnp_hist_spec\s*\{\s*ekpnp_hist_axis\s+a,\s*b;\s*\}\s*ekpnp_hist_spec;", code)
    assert C.sizeof(pkg.HistAxis) == 24 and C.sizeof(pkg.HistSpec) == 48
    assert [n for n, _ in pkg.HistAxis._fields_] == ["value", "n", "lo", "hi"] and [n for n, _ in pkg.HistSpec._fields_] == ["a", "b"]
    for cls in (pkg.Solver, pkg.Group):
        for name in ["hist_planes", "value_range"] + ["hist_" + v for v in VERBS]:
            assert hasattr(cls, name), (cls.__name__, name)
    s = pkg.hist_spec(("q", 129, -1.5, 2.5))
    assert (s.a.value, s.a.n, s.a.lo, s.a.hi, s.b.n) == (11, 129, -1.5, 2.5, 0) and s.cells == 131 and s.cell_shape == (131,)
    s = pkg.hist_spec(("uz", 7, -1.0, 1.0), (10, 5, 0.0, 1.0))
    assert (s.a.value, s.b.value, s.b.n) == (6, 10, 5) and s.cells == 9 * 7 and s.cell_shape == (9, 7)
    e = pkg.hist_edges(("uz", 4, -1.0, 1.0))
    assert e.tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0]


def test_the_file_header_is_documented():
    text = " ".join(re.sub(r"\n\s*\*", " ", _header()).split())
    assert ("# ekpnp hist nx <nx> ny <ny> nz <nz> a <name> <n> <lo> <hi> [b <name> <n> <lo> <hi>] z_lo <z> z_hi <z> recorded <r> "
            "dropped <d>") in text
    assert "step time nonfinite cell cell ..." in text
    main = open(os.path.join(ROOT, "ek-pnp-3d_amd", "csrc", "ekpnp_main.cpp")).read()
    for flag in ("--hist-every", "--hist-value", "--hist-bins", "--hist-range", "--hist-value2", "--hist-bins2", "--hist-range2", "--hist-planes"):
        assert flag in main, flag


GOOD_A = ("uz", 8, -1.0, 1.0)


@pytest.mark.parametrize("a, b, number", [
    (("uz", 0, -1.0, 1.0), None, "n = 0"),
    (("uz", -3, -1.0, 1.0), None, "-3"),
    (("uz", 8, 1.0, 1.0), None, "hi = 1 "),                 # hi <= lo
    (("uz", 8, 2.5, -0.25), None, "-0.25"),
    (("uz", 8, float("-inf"), 1.0), None, "lo = -inf"),      # a non-finite bound
    (("uz", 8, -1.0, float("inf")), None, "hi = inf"),
    (("uz", 8, float("nan"), 1.0), None, "lo = nan"),
    (("uz", 8, -1e308, 1e308), None, "inf"),                 # hi - lo overflows
    (("uz", 8, 0.0, 5e-324), None, "4.9406564584124654e-324"),  # n / (hi - lo) overflows
    ((12, 8, -1.0, 1.0), None, "12"),                        # value id outside 0 .. 11
    ((-1, 8, -1.0, 1.0), None, "-1"),
    (GOOD_A, (12, 8, -1.0, 1.0), "12"),
    (GOOD_A, ("T", 8, 3.0, 3.0), "hi = 3 "),
    (GOOD_A, ("T", -2, 0.0, 1.0), "-2"),
    (("uz", 4097, -1.0, 1.0), None, "4097"),                 # a.n * max(b.n, 1) <= 4096
    (("uz", 64, -1.0, 1.0), ("T", 65, 0.0, 1.0), "4160"),
    (("uz", 128, -1.0, 1.0), ("q", 64, 0.0, 1.0), "8192"),
])
def test_bad_specs_are_refused_with_the_offending_number(pkg, a, b, number):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    spec = pkg.hist_spec(a, b)
    assert lib.ekpnp_hist_spec_check(C.byref(p), C.byref(spec)) == INVALID
    msg = lib.ekpnp_last_error(None).decode()
    assert number in msg, msg
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.hist_spec_check(p, spec)
    assert "status 1" in str(e.value) and number in str(e.value), str(e.value)


@pytest.mark.parametrize("z_lo, z_hi, capacity, number", [
    (7, 3, 4, "7"),          # z_lo > z_hi
    (0, 13, 4, "13"),        # z_hi >= nz
    (5, 40, 4, "40"),
    (-1, 3, 4, "-1"),
    (1, 11, 0, "capacity = 0"),
    (1, 11, -5, "-5"),
])
def test_bad_planes_and_capacities_are_refused_with_the_offending_number(pkg, z_lo, z_hi, capacity, number):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    assert lib.ekpnp_hist_range_check(C.byref(p), z_lo, z_hi, capacity) == INVALID
    msg = lib.ekpnp_last_error(None).decode()
    assert number in msg, msg
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.hist_spec_check(p, pkg.hist_spec(GOOD_A), planes=(z_lo, z_hi), capacity=capacity)
    assert "status 1" in str(e.value) and number in str(e.value), str(e.value)


def test_good_specs_are_accepted(pkg):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    for value in pkg.HIST_VALUES:
        for n in (1, 2, 129, 4096):
            spec = pkg.hist_spec((value, n, -1e-3, 2e-3))
            assert lib.ekpnp_hist_spec_check(C.byref(p), C.byref(spec)) == 0, lib.ekpnp_last_error(None)
        for na, nb in ((7, 5), (64, 64), (1, 4096), (4096, 1), (2, 2048)):
            spec = pkg.hist_spec((value, na, -1e300, 1e300), ("q", nb, 0.0, 1e-300))
            assert lib.ekpnp_hist_spec_check(C.byref(p), C.byref(spec)) == 0, lib.ekpnp_last_error(None)
            assert spec.cells == (na + 2) * (nb + 2)
    for z_lo, z_hi, cap in ((0, 12, 1), (1, 11, 1000), (6, 6, 3), (12, 12, 1)):
        assert lib.ekpnp_hist_range_check(C.byref(p), z_lo, z_hi, cap) == 0, lib.ekpnp_last_error(None)
    assert pkg.hist_spec_check(p, pkg.hist_spec(GOOD_A, ("T", 8, 0.0, 1.0)), planes=(1, 11), capacity=8).b.n == 8


def test_null_arguments_are_refused_not_dereferenced(pkg):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    spec = pkg.hist_spec(GOOD_A)
    buf = np.zeros(64)
    ptr = buf.ctypes.data_as(C.c_void_p)
    a, b = C.c_int64(), C.c_int64()
    assert lib.ekpnp_hist_spec_check(None, C.byref(spec)) == INVALID
    assert lib.ekpnp_hist_spec_check(C.byref(p), None) == INVALID
    assert lib.ekpnp_hist_range_check(None, 1, 2, 3) == INVALID
    for prefix in ("ekpnp_", "ekpnp_group_"):
        assert getattr(lib, prefix + "hist_planes")(None, C.byref(spec), ptr, ptr) == INVALID
        assert getattr(lib, prefix + "value_range")(None, 6, ptr, ptr) == INVALID
        assert getattr(lib, prefix + "hist_arm")(None, C.byref(spec), 1, 2, 4) == INVALID
        assert getattr(lib, prefix + "hist_disarm")(None) == INVALID
        assert getattr(lib, prefix + "hist_record")(None, 1, 0.0) == INVALID
        assert getattr(lib, prefix + "hist_count")(None, C.byref(a), C.byref(b)) == INVALID
        assert getattr(lib, prefix + "hist_read")(None, 0, 1, None, None, ptr) == INVALID
        assert getattr(lib, prefix + "hist_save")(None, b"/nonexistent/hist.dat") == INVALID
    assert (buf == 0.0).all()


def definition(lo, hi, n, v):
    """include/ekpnp.h transcribed into numpy float64: every operation rounded once"""
    lo, hi = np.float64(lo), np.float64(hi)
    v = np.asarray(v, dtype=np.float64)
    scale = np.float64(n) / (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        d = v - lo
        s = d * scale
        inside = ~(v != v) & ~(v < lo) & ~(v >= hi)
        k = np.minimum(np.where(inside, s, 0.0).astype(np.int64), n - 1)  # astype truncates towards zero, as (int) does
    return np.where(v != v, -1, np.where(v < lo, 0, np.where(v >= hi, n + 1, 1 + k))).astype(np.int32)


def edge_values(lo, hi, n):
    """lo, hi, the double below hi, every edge lo + k (hi - lo) / n and its two neighbours, -0.0, +-Inf, NaN"""
    lo, hi = np.float64(lo), np.float64(hi)
    edges = lo + np.arange(n + 1, dtype=np.float64) * (hi - lo) / n
    return np.concatenate([[lo, hi, np.nextafter(hi, lo), np.nextafter(lo, -np.inf), -0.0, 0.0, np.inf, -np.inf, np.nan], edges,
                           np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])


@pytest.mark.parametrize("n", [1, 2, 7, 4096])
@pytest.mark.parametrize("lo, hi", [(-1.0, 1.0), (-3.7e-4, 9.1e-4), (0.1, 0.7), (-0.0, 3.0)])
def test_hist_bin_is_its_definition(pkg, n, lo, hi):
    rng = np.random.default_rng(1000 * n + int(1e3 * hi))
    width = hi - lo
    v = np.concatenate([edge_values(lo, hi, n), rng.uniform(lo - 0.25 * width, hi + 0.25 * width, size=100_000)])
    got = pkg.hist_bin(lo, hi, n, v)
    want = definition(lo, hi, n, v)
    assert got.dtype == np.int32 and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    # what the definition says in words
    assert pkg.hist_bin(lo, hi, n, lo) == 1 and pkg.hist_bin(lo, hi, n, hi) == n + 1 and pkg.hist_bin(lo, hi, n, np.nextafter(hi, lo)) == n
    assert pkg.hist_bin(lo, hi, n, np.nextafter(lo, -np.inf)) == 0
    assert pkg.hist_bin(lo, hi, n, float("inf")) == n + 1 and pkg.hist_bin(lo, hi, n, float("-inf")) == 0 and pkg.hist_bin(lo, hi, n, float("nan")) == -1
    assert pkg.hist_bin(lo, hi, n, -0.0) == pkg.hist_bin(lo, hi, n, 0.0)
    assert got.min() == -1 and got.max() == n + 1 and set(np.unique(got)) == set(range(-1, n + 2))  # every index occurs
