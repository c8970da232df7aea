"""CPU tests of sampling the fields at the tracers and of the tracks' spec (csrc/tracers.hip; include/ekpnp.h: ekpnp_tracers_sample_host,
ekpnp_tracers_values_check, ekpnp_tracks_spec_check): the host-only entry points, which ARE the definitions the device is held against
in tests/test_tracers_sample_gpu.py.  No device is needed.

ekpnp_tracers_sample_host is compared with a numpy transcription of the header's text (tests/_tracers_sample_ref.py, on the stencil and
the value of tests/_tracers_ref.py) on the float64 BIT PATTERN; no tolerance appears anywhere.  The exact case uses dyadic numbers, so
every difference, product and sum is exact and the expected value is known in closed form."""
import ctypes as C
import os

import numpy as np
import pytest

import _tracers_ref as T
import _tracers_sample_ref as S

NEW = ["ekpnp_tracers_values_check", "ekpnp_tracers_sample_host", "ekpnp_tracers_sample_device", "ekpnp_tracers_sample", "ekpnp_tracks_spec_check",
       "ekpnp_tracks_arm", "ekpnp_tracks_disarm", "ekpnp_tracks_record", "ekpnp_tracks_count", "ekpnp_tracks_read", "ekpnp_tracks_save"]
METHODS = ["tracers_sample", "tracers_sample_into", "tracks_arm", "tracks_disarm", "tracks_record", "tracks_count", "tracks_read", "tracks_save"]


@pytest.fixture(scope="module")
def fields():
    return {k: S.all_fields(s, 900 + i) for i, (k, s) in enumerate(S.SHAPES.items())}


# ---- 1. the interface ------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_mirrored(pkg):
    lib = pkg.load_library()
    for name in NEW:
        assert name in pkg.exported_symbols()
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    assert not [n for n in pkg.exported_symbols() if n.startswith("ekpnp_group_tracks") or n.startswith("ekpnp_group_tracers")]
    for m in METHODS:
        assert hasattr(pkg.Solver, m), m
    assert not [m for m in dir(pkg.Group) if "tracks" in m]
    for f in ("tracers_sample_host", "tracers_values_check", "tracks_spec", "tracks_spec_check"):
        assert callable(getattr(pkg, f)), f
    assert (pkg.TRACERS_Q, pkg.TRACERS_MAX_VALUES, pkg.TRACERS_MAX_TRACKS) == (11, 12, 1024)
    assert pkg.TRACERS_VALUES == S.NAMES and pkg.TRACERS_VALUES[:11] == pkg.FIELDS
    assert C.sizeof(pkg.TracksSpec) == 8 + 4 * 12 + 4 * 1024
    assert [getattr(pkg.TracksSpec, n).offset for n in ("ntags", "nvalues", "values", "ids")] == [0, 4, 8, 56]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ekpnp.h")).read()
    for text in ("#define EKPNP_TRACERS_Q 11", "#define EKPNP_TRACERS_MAX_VALUES 12", "#define EKPNP_TRACERS_MAX_TRACKS 1024"):
        assert text in hdr, text


# ---- 2. the definition against its transcription --------------------------------------------------------------------------

@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_sample_host_equals_the_transcription(pkg, fields, shape):
    dims = S.SHAPES[shape]
    p = pkg.default_params(*dims)
    f = fields[shape]
    for n in S.NS:
        x, y, z = T.special_cloud(dims, n, 40 + n)
        want = S.sample(dims, f, S.NAMES, x, y, z)
        got = pkg.tracers_sample_host(p, S.NAMES, f, x, y, z)
        assert S.same_sample(got, want), (shape, n)
        if n >= 1000:   # the wrap in x and in y, both plates, fz == 1 and a lost particle are in it
            assert np.isnan(want[:, 12]).all() and not np.isnan(np.delete(want, 12, axis=1)).any()
            assert x[1] > dims[0] - 1 and y[2] > dims[1] - 1 and z[3] == 0.0 and z[4] == dims[2] - 1
        # the order of the names is the order of the rows; ids and names are the same thing; a subset reads only its arrays
        order = ["q", "T", "ux", "rho"]
        got = pkg.tracers_sample_host(p, [pkg.TRACERS_VALUE_ID[v] for v in order], f, x, y, z)
        assert S.same_sample(got, want[[S.NAMES.index(v) for v in order]]), (shape, n)
        got = pkg.tracers_sample_host(p, "q", {"c": f["c"], "cn": f["cn"]}, x, y, z)
        assert got.shape == (1, n) and S.same_sample(got, want[11:12])
        got = pkg.tracers_sample_host(p, ["uz"], {"uz": f["uz"]}, x, y, z)
        assert S.same_sample(got, want[6:7])


def test_q_is_formed_per_node_not_from_two_interpolations(pkg, fields):
    dims = S.SHAPES["W"]
    p = pkg.default_params(*dims)
    f = fields["W"]
    x, y, z = T.special_cloud(dims, 4097, 41)
    c, cn, q = pkg.tracers_sample_host(p, ["c", "cn", "q"], f, x, y, z)
    alive = ~np.isnan(x)
    assert not np.array_equal(T.bits((c - cn)[alive]), T.bits(q[alive]))   # the other order of the operations rounds differently somewhere
    assert np.abs((c - cn)[alive] - q[alive]).max() < 1e-14


def test_an_affine_field_is_sampled_exactly(pkg):
    """a = 3 + x/2 + y/4 + 2 z at the nodes, positions on multiples of 1/8 away from the periodic seam: every operation is exact"""
    dims = S.SHAPES["O"]
    nx, ny, nz = dims
    p = pkg.default_params(*dims)
    k, j, i = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64), np.arange(nx, dtype=np.float64), indexing="ij")
    a = 3.0 + 0.5 * i + 0.25 * j + 2.0 * k
    b = 1.0 - 0.125 * i + 4.0 * j + 0.5 * k
    rng = np.random.default_rng(7)
    n = 1000
    x = rng.integers(0, 8 * (nx - 1), n) / 8.0
    y = rng.integers(0, 8 * (ny - 1), n) / 8.0
    z = rng.integers(0, 8 * (nz - 1) + 1, n) / 8.0
    z[:3] = (0.0, nz - 1.0, nz - 1.125)
    got = pkg.tracers_sample_host(p, ["T", "c", "cn", "q"], {"T": a, "c": a, "cn": b}, x, y, z)
    fa = 3.0 + 0.5 * x + 0.25 * y + 2.0 * z
    fb = 1.0 - 0.125 * x + 4.0 * y + 0.5 * z
    for row, want in zip(got, (fa, fa, fb, fa - fb)):
        assert T.same(row, want)


def test_a_nan_node_reaches_exactly_the_particles_whose_stencil_holds_it(pkg, fields):
    dims = S.SHAPES["R"]
    nx, ny, nz = dims
    p = pkg.default_params(*dims)
    n = 4097
    x, y, z = T.special_cloud(dims, n, 43)
    alive = np.flatnonzero(~np.isnan(x))
    i0, i1, _, j0, j1, _, k0, k1, _ = T._stencil(dims, x[alive], y[alive], z[alive])
    # nodes (k, j, i): the first one particle 0 loads; one that particle 1 reaches through the wrap in x, one that particle 2
    # reaches through the wrap in y; one on the upper plate, under particle 4 (fz == 1)
    nodes = (((int(k0[0]), int(j0[0]), int(i0[0])), np.nan, 0), ((2, 1, 0), np.nan, 1), ((3, 0, 3), np.inf, 2), ((nz - 1, 5, 6), np.inf, 4))
    for node, bad, particle in nodes:
        f = {name: np.array(fields["R"][name]) for name in ("c", "cn", "T")}
        f["T"][node] = bad
        f["cn"][node] = bad
        hit = np.zeros(n, dtype=bool)
        hit[alive] = ((k0 == node[0]) | (k1 == node[0])) & ((j0 == node[1]) | (j1 == node[1])) & ((i0 == node[2]) | (i1 == node[2]))
        assert hit[particle] and hit.sum() < 40, node
        got = pkg.tracers_sample_host(p, ["T", "q", "c"], f, x, y, z)
        clean = pkg.tracers_sample_host(p, ["T", "q", "c"], fields["R"], x, y, z)
        for row in (0, 1):
            touched = ~np.isfinite(got[row])
            touched[np.isnan(x)] = False
            assert np.array_equal(touched, hit), (node, row)
            assert np.array_equal(T.bits(got[row][~hit]), T.bits(clean[row][~hit]))
        assert S.same_sample(got[2], clean[2])   # c holds no bad node
        assert np.isnan(got[:, np.isnan(x)]).all()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------

def _refused(pkg, call):
    with pytest.raises(pkg.EkpnpError) as e:
        call()
    assert "status 1" in str(e.value)
    return str(e.value)


def test_bad_values_are_refused_with_the_offending_number(pkg, fields):
    dims = S.SHAPES["O"]
    p = pkg.default_params(*dims)
    f = fields["O"]
    x = np.array([1.5])
    assert pkg.tracers_values_check(p, S.NAMES).tolist() == list(range(12))
    assert pkg.tracers_values_check(p, "q").tolist() == [11]
    for check in (lambda v: pkg.tracers_values_check(p, v), lambda v: pkg.tracers_sample_host(p, v, f, x, x, x)):
        assert "nvalues = 0" in _refused(pkg, lambda: check([]))
        assert "nvalues = 13" in _refused(pkg, lambda: check(list(range(12)) + [0]))
        assert "value id 12" in _refused(pkg, lambda: check([0, 12]))
        assert "value id -1" in _refused(pkg, lambda: check([-1]))
        assert "value id 4 is named twice" in _refused(pkg, lambda: check(["ux", "T", 4]))
    thin = pkg.default_params(8, 8, 8)
    thin.nz = 2
    flat = {"T": np.zeros((2, 8, 8))}
    assert "nz = 2" in _refused(pkg, lambda: pkg.tracers_values_check(thin, ["T"]))
    assert "nz = 2" in _refused(pkg, lambda: pkg.tracers_sample_host(thin, ["T"], flat, x, x, x))
    assert "value q is named and its array is NULL" in _refused(pkg, lambda: pkg.tracers_sample_host(p, ["c", "q"], {"c": f["c"]}, x, x, x))
    assert "value Ez is named and its array is NULL" in _refused(pkg, lambda: pkg.tracers_sample_host(p, ["Ez"], {"c": f["c"]}, x, x, x))
    L = pkg.load_library()
    ids = np.array([0], dtype=np.int32)
    out = np.zeros(1)
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    arrays = (C.c_void_p * 11)(*[f[n].ctypes.data for n in pkg.FIELDS])
    good = [C.byref(p), 1, ptr(ids), arrays, 1, ptr(x), ptr(x), ptr(x), ptr(out)]
    assert L.ekpnp_tracers_sample_host(*good) == 0
    for k in (0, 2, 3, 5, 6, 7, 8):
        bad = list(good)
        bad[k] = None
        assert L.ekpnp_tracers_sample_host(*bad) == 1 and b"NULL" in L.ekpnp_last_error(None), k
    bad = list(good)
    bad[4] = -1
    assert L.ekpnp_tracers_sample_host(*bad) == 1 and b"n = -1" in L.ekpnp_last_error(None)
    bad[4] = 0   # no particle: nothing is read, nothing is written
    bad[5] = bad[8] = None
    assert L.ekpnp_tracers_sample_host(*bad) == 0


def test_bad_track_specs_are_refused_with_the_offending_number(pkg):
    p = pkg.default_params(*S.SHAPES["W"])
    n = 1000
    good = pkg.tracks_spec(ids=[7, 999, 0, 500], values=["T", "q"])
    assert pkg.tracks_spec_check(p, n, good) is good and good.names() == ["T", "q"] and (good.ntags, good.nvalues) == (4, 2)
    assert pkg.tracks_spec_check(p, n, pkg.tracks_spec(ids=[3])).nvalues == 0   # positions only
    assert pkg.tracks_spec_check(p, 1024, pkg.tracks_spec(ids=np.arange(1024)[::-1], values=S.NAMES)).ntags == 1024
    check = lambda spec, m=n: _refused(pkg, lambda: pkg.tracks_spec_check(p, m, spec))
    assert "id 999 is tagged twice" in check(pkg.tracks_spec(ids=[7, 999, 0, 999]))
    assert "id 1000" in check(pkg.tracks_spec(ids=[7, 1000])) and "0 .. 999" in check(pkg.tracks_spec(ids=[7, 1000]))
    assert "id -1" in check(pkg.tracks_spec(ids=[-1]))
    assert "ntags = 0" in check(pkg.tracks_spec(ids=[]))
    big = pkg.tracks_spec(ids=[1])
    big.ntags = 1025
    assert "ntags = 1025" in check(big, 5000)
    assert "value id 12" in check(pkg.tracks_spec(ids=[1], values=[12]))
    assert "value id 3 is named twice" in check(pkg.tracks_spec(ids=[1], values=[3, 3]))
    bad = pkg.tracks_spec(ids=[1])
    bad.nvalues = 13
    assert "nvalues = 13" in check(bad)
    bad.nvalues = -1
    assert "nvalues = -1" in check(bad)
    assert "n = 0" in check(good, 0)
    L = pkg.load_library()
    assert L.ekpnp_tracks_spec_check(C.byref(p), n, None) == 1 and b"NULL" in L.ekpnp_last_error(None)
    assert L.ekpnp_tracks_spec_check(None, n, C.byref(good)) == 1 and b"NULL" in L.ekpnp_last_error(None)
