"""CPU tests of the field diagnostics past the size thresholds of their kernels (csrc/stats.hip, monitor.hip, modes.hip, hist.hip,
diag.hip, section.hip, spectrum.hip, snapshot.hip): what can be held without a device.  The shapes of tests/_diag_sizes.py sit on the
side of each threshold they are there for, by the constants the sources have today (a retuned tile size fails here; it does not
silently un-test a path); the exact references the GPU file (tests/test_diag_sizes_gpu.py) compares the device with are held against
brute force on a tiny lattice; and the field builders keep the placements the GPU tests rely on.  Every comparison is of integers,
of bit patterns or with ==, except where rfft2_power is held against the long-double transform of tests/test_spectrum_gpu.py."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _diag_sizes as Z
import test_section_gpu as TSEC
import test_spectrum_gpu as TSPEC

TINY = (5, 3, 4)


# ---- 0. the shapes and the thresholds ---------------------------------------------------------------------------------------------

def test_the_sources_have_the_tile_sizes_the_shapes_were_chosen_for():
    for name, want in Z.CONSTANTS.items():
        src = Z.source_constants(name)
        for k, v in want.items():
            assert src.get(k) == v, (name, k, src.get(k))
    text = {n: open(Z.os.path.join(Z.CSRC, n), encoding="utf-8").read() for n in Z.CONSTANTS if n.endswith(".hip")}
    # the literals behind FINISH_BATCH, HIST_BATCH, FINAL_THREADS, RANGE_LANES, SEC_X_ROWS and the 256 of plate_blocks
    assert text["monitor.hip"].count("for (int b0 = 0; b0 < nwg; b0 += 16)") == 1 and "double v[16];" in text["monitor.hip"]
    assert text["modes.hip"].count("for (int b0 = 0; b0 < nwg; b0 += 16)") == 1
    assert "for (int b0 = 0; b0 < nwg; b0 += 8)" in text["hist.hip"]
    assert "for (int b = threadIdx.x; b < nwg; b += 64)" in text["hist.hip"] and "__launch_bounds__(64) k_range_finish" in text["hist.hip"]
    assert "hipLaunchKernelGGL(k_range_finish, dim3(c.nzl), dim3(64)" in text["hist.hip"]
    assert "HIST_CHUNK0 * (((long long)stride + 2047) / 2048)" in text["hist.hip"]
    assert "((long long)c.plane + HIST_THREADS * HIST_LOADS - 1) / (HIST_THREADS * HIST_LOADS)" in text["hist.hip"]
    assert text["diag.hip"].count("(n + 255) / 256 < DIAG_BLOCKS") == 2 and "(c.plane + 255) / 256 < DIAG_BLOCKS" in text["diag.hip"]
    assert "for (int i = threadIdx.x; i < n; i += blockDim.x)" in text["diag.hip"]            # k_final ...
    assert text["diag.hip"].count("dim3(1), dim3(256), 0, c.stream, scratch, nb") == 3            # ... of 256 threads
    assert "for (int i = threadIdx.x; i < a.nb; i += blockDim.x)" in text["monitor.hip"]
    assert "hipLaunchKernelGGL(k_monitor_finish, dim3(1), dim3(256)" in text["monitor.hip"]
    assert "const bool in_lds = nitems <= MON_LDS_PLANES;" in text["monitor.hip"] and "const int nitems = a.nzl * MON_NV;" in text["monitor.hip"]
    assert "constexpr int ROWS = PAIR ? 32 : 64;" in text["section.hip"]
    assert "int xchunks;          // ceil(X / SNAP_LANES)" in text["snapshot.hip"]
    assert Z.K["MON_PLATE_BLOCKS"] == Z.K["DIAG_BLOCKS"] and Z.K["STATS_CHUNK"] == Z.K["MON_CHUNK"] == Z.K["MODE_CHUNK"]
    assert Z.K["HIST_CHUNK0"] == 2 * Z.K["HIST_THREADS"] * Z.K["HIST_LOADS"]


def test_each_shape_sits_on_the_side_of_its_threshold_written_in_the_table():
    S, P = Z.SHAPES, {k: Z.plane(s) for k, s in Z.SHAPES.items()}
    chunk, batch = Z.K["MON_CHUNK"], Z.FINISH_BATCH
    # A: the last size before the second batch - 16 and 8 workgroups, all full
    assert P["A"] == 65536 == batch * chunk == Z.HIST_BATCH * Z.K["HIST_CHUNK0"]
    assert Z.chunk_workgroups(S["A"]) == 16 and Z.hist_workgroups(S["A"], 131) == 8 and S["A"][0] % 64 == 0   # ROW64
    # B: one workgroup into the second batch, 256 live nodes in it; rows no multiple of 64
    assert P["B"] == 65792 and Z.chunk_workgroups(S["B"]) == 17 and Z.hist_workgroups(S["B"], 131) == 9
    assert P["B"] - 16 * chunk == 256 == P["B"] - 8 * Z.K["HIST_CHUNK0"] and S["B"][0] % 64 != 0
    assert Z.plate_blocks(P["A"]) == 256 == Z.FINAL_THREADS and Z.plate_blocks(P["B"]) == 257   # k_final's second round: one partial
    # C: 33 = 16 + 16 + 1 and 17 = 8 + 8 + 1 workgroups; an odd plane
    assert P["C"] == 131407 and P["C"] % 2 == 1 and Z.chunk_workgroups(S["C"]) == 33 and Z.hist_workgroups(S["C"], 131) == 17
    assert [Z.ceil_div(w, batch) for w in (16, 17, 33, 65)] == [1, 2, 3, 5] and [Z.ceil_div(w, Z.HIST_BATCH) for w in (8, 9, 17, 33)] == [1, 2, 3, 5]
    nx, ny, _ = S["C"]
    assert Z.ceil_div(nx, Z.K["SEC_Y_THREADS"]) == 2                                                 # k_section_y: two workgroups along x
    assert [Z.ceil_div(ny, r) for r in Z.SEC_X_ROWS] == [7, 13]                                      # k_section_x: row tiles
    assert divmod(ny, Z.K["SEC_RUN"]) == (6, 13) and Z.ceil_div(nx, Z.K["SEC_RUN"]) == 6             # runs across y: 6 and a tail of 13; across x: 6
    assert Z.ceil_div(nx, Z.K["SNAP_LANES"]) == 6 and nx // Z.K["SNAP_LANES"] > 2
    assert all(nx % k and ny % k for k in range(2, 20))                                              # 331 and 397 are prime: only cx = cy = 1
    # D: the grid-stride round and the second round of k_range_finish's lanes
    assert P["D"] == 262600 and Z.ceil_div(P["D"], 256) == 1026 and Z.plate_blocks(P["D"]) == 1024 and P["D"] - 1024 * 256 == 456
    assert Z.range_workgroups(S["D"]) == 65 == Z.RANGE_LANES + 1 and Z.range_workgroups(S["C"]) == 33 and Z.chunk_workgroups(S["D"]) == 65
    assert Z.hist_workgroups(S["D"], 131) == 33
    assert all(Z.plane(S[k]) * S[k][2] > 1024 * 256 for k in "BCD") and P["A"] * S["A"][2] == 1024 * 256   # k_max_uz: one round on A exactly
    # the chunks of the histograms: 8192, 16 384 and 24 576 nodes, 2 .. 12 tiles
    strides = {k: Z.hist_stride(a, b) for k, (a, b, _) in Z.HIST_SPECS.items()}
    assert strides == {"uz128": 131, "T2048": 2051, "q4096": 4099, "q_uz": 4357, "uz_T": 1157}
    assert {k: Z.hist_chunk(s) for k, s in strides.items()} == {"uz128": 8192, "T2048": 16384, "q4096": 24576, "q_uz": 24576, "uz_T": 8192}
    tiles = {k: (Z.hist_tiles(strides[k], narr, 2), Z.hist_tiles(strides[k], narr, 1)) for k, (_, _, narr) in Z.HIST_SPECS.items()}
    assert tiles == {"uz128": (1, 2), "T2048": (2, 4), "q4096": (6, 12), "q_uz": (12, 24), "uz_T": (2, 4)}
    assert all(P[k] >= 24576 for k in "CD")
    assert {k: Z.hist_workgroups(S["C"], s) for k, s in strides.items()} == {"uz128": 17, "T2048": 9, "q4096": 6, "q_uz": 6, "uz_T": 17}
    assert {k: Z.hist_workgroups(S["D"], s) for k, s in strides.items()} == {"uz128": 33, "T2048": 17, "q4096": 11, "q_uz": 11, "uz_T": 33}
    # E: LDS exactly not overfull, then one plane past it
    assert S["E585"][2] * Z.K["MON_NV"] == 4095 <= Z.K["MON_LDS_PLANES"] < S["E586"][2] * Z.K["MON_NV"] == 4102
    assert Z.K["MON_LDS_PLANES"] // Z.K["MON_NV"] == 585
    # F: a batch of 15, so sixteen planes make 15 + 1
    nx, ny, nz = S["F"]
    assert ny * (nx // 2 + 1) * 16 > 4 << 20 and Z.spectrum_batch(S["F"]) == 15 and nz == Z.K["EKPNP_MAX_SPECTRUM_PLANES"] == 16
    assert all(Z.spectrum_batch(S[k]) == 16 for k in "ABCD") and Z.spectrum_batch((512, 512, 4)) == 16
    # S: two uneven slabs of C's plane
    assert S["S"][:2] == S["C"][:2] and [S["S"][2] * r // 2 for r in (0, 1, 2)] == [0, 4, 9]
    # the byte counts the GPU file asserts, once by hand
    assert Z.stats_bytes(S["C"], 4) == (4 * 33 * 24 + 2 * 24 * 4) * 8 and Z.monitor_bytes(S["D"], 4) == (4 * 1024 + 4 * 65 * 7 + 4 * 7 + 16) * 8
    assert Z.modes_bytes(S["B"], 4) == (4 * 17 * 32 + 16 * 4 * 2 + 64 * (257 + 256)) * 8
    assert Z.hist_bytes(S["C"], 4, [131]) == 4 * 17 * 131 * 4 + 4 * 131 * 8


def test_the_library_has_the_parameters_the_references_assume(pkg):
    p = pkg.default_params(*Z.SHAPES["D"])
    assert p.rho0 == Z.RHO0 and float(p.rho0).is_integer() and p.n_lattices == 4
    assert pkg.FIELDS == Z.FIELDS and pkg.PROFILE_NAMES == Z.PROFILES and len(pkg.MONITOR_NAMES) == Z.K["EKPNP_NMONITORS"]
    assert pkg.MONITOR_NAMES == ["current_top", "current_bottom", "dTdz_bottom", "dTdz_top", "uz_max", "u_u", "q", "q_q", "uz_T", "rho_dev", "nonfinite"]
    for k in "ABCDS":
        q = pkg.default_params(*Z.SHAPES[k])
        pkg.modes_spec_check(q, pkg.modes_spec("uz", Z.modes_of(Z.SHAPES[k])))
        assert len(set(Z.modes_of(Z.SHAPES[k]))) == 16
        for a, b, _ in Z.HIST_SPECS.values():
            pkg.hist_spec_check(q, pkg.hist_spec(a, b), planes=(1, 2))
        for across in ("x", "y"):
            for lo, hi in Z.section_ranges(Z.SHAPES[k], across).values():
                pkg.section_spec_check(q, pkg.section_spec(None, across, (lo, hi)))
    with pytest.raises(ValueError):   # six planes cannot be cut into two slabs: a slab needs four planes
        pkg.slab_extent(6, 0, 2)
    assert [pkg.slab_extent(9, r, 2) for r in (0, 1)] == [(0, 4), (4, 5)]


# ---- 1. the builders ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["A", "B", "C", "D", "E585", "E586"])
def test_the_dyadic_fields_keep_their_placements(key):
    shape = Z.SHAPES[key]
    nx, ny, nz = shape
    P = nx * ny
    pl = Z.plants(shape)
    assert pl["last"] == (nz - 1, P - 1) and (("batch2" in pl) == (P > 65536))
    if "batch2" in pl:
        assert pl["batch2"] == (nz - 2, 65536) and pl["batch2"][1] // Z.K["MON_CHUNK"] == Z.FINISH_BATCH
    assert pl["last"][1] // Z.K["MON_CHUNK"] == Z.chunk_workgroups(shape) - 1
    if key == "D":
        assert pl["last"][1] >= 262144
    if key == "E586":
        assert pl["last"][0] == 585 and Z.nan_node(shape) == (585, P - 1)
    if nz == 4:
        assert Z.nan_node(shape) == (2, P - 1)
    seen = []
    for variant in (0, 1):
        f = Z.dyadic_fields(shape, 7, variant, nan=Z.nan_node(shape) if variant else None)
        assert list(f) == Z.FIELDS
        uz, dev = f["uz"].reshape(nz, P), np.abs(f["rho"] - Z.RHO0).reshape(nz, P)
        at_uz, at_rho = np.argwhere(uz == uz.max()).tolist(), np.argwhere(dev == dev.max()).tolist()
        assert len(at_uz) == 1 and len(at_rho) == 1 and uz.max() == Z.PLANT_UZ and dev.max() == Z.PLANT_RHO   # unique
        seen.append((tuple(at_uz[0]), tuple(at_rho[0])))
        assert np.isnan(f["c"]).sum() == variant and all(not np.isnan(v).any() for n, v in f.items() if n != "c")
        for n, v in f.items():
            i = Z.to_int(v)                                                     # on the grid
            lo = i.min() - (Z.Q * 1000 if n == "rho" else 0)
            assert lo >= -Z.Q and (n in ("uz", "rho") or i.max() <= Z.Q)
        assert not np.array_equal(f["ux"][0], f["ux"][1]) and not np.array_equal(f["ux"], f["uy"])   # planes and fields differ
    other = pl.get("batch2", (1, P - 1))
    assert seen == [(pl["last"], other), (other, pl["last"])]                    # variant 1 swaps the two nodes
    assert Z.worst_case_quanta(shape) < 2 ** 53


def test_the_worst_case_sum_of_shape_d_stays_below_2_53_quanta():
    assert Z.worst_case_quanta(Z.SHAPES["D"]) == 2 * 262600 * 1002 * 2 ** 20 < 2 ** 50
    f = Z.dyadic_fields(Z.SHAPES["D"], 7)
    i = {n: Z.to_int(v) for n, v in f.items()}
    q = np.abs(i["c"]) + np.abs(i["cn"])
    worst = max(int((np.abs(a) * np.abs(b)).sum(axis=(1, 2)).max()) for a, b in ((q, q), (q, i["Ez"]), (i["uz"], i["T"]), (i["rho"], np.int64(Z.Q))))
    assert 2 * worst <= Z.worst_case_quanta(Z.SHAPES["D"])


@pytest.mark.parametrize("key", ["C", "D"])
def test_the_random_fields_keep_the_extremes_of_the_value_range(key):
    shape = Z.SHAPES[key]
    nx, ny, nz = shape
    P = nx * ny
    top = Z.range_top_node(shape)
    assert top == (262144 if key == "D" else 65536) and top // 4096 == (64 if key == "D" else 16) and (P - 1) // 4096 == Z.range_workgroups(shape) - 1
    f = Z.random_fields(shape, 3)
    for name in ("uz", "q"):
        v = Z.value(f, name).reshape(nz, P)
        for z in range(nz):
            assert np.flatnonzero(v[z] == v[z].min()).tolist() == [P - 1] and np.flatnonzero(v[z] == v[z].max()).tolist() == [top]
    assert all(np.isfinite(v).all() for v in f.values())
    assert not np.array_equal(f["uz"] * 1024.0, np.rint(f["uz"] * 1024.0))      # not dyadic


# ---- 2. the references against brute force on a tiny lattice ------------------------------------------------------------------------

def _fsum(a):
    return math.fsum(np.asarray(a, dtype=np.float64).ravel().tolist())


def test_plane_sums_exact_against_brute_force():
    f = Z.dyadic_fields(TINY, 5)
    got = Z.plane_sums_exact(f)
    assert got.shape == (24, TINY[2])
    q = f["c"] - f["cn"]                                                          # exact: dyadic
    v = dict(f, q=q)
    for k, name in enumerate(Z.PROFILES):
        for z in range(TINY[2]):
            terms = v[name][z] if k < 11 else v[name.split("_")[0]][z] * v[name.split("_")[1]][z]   # exact products
            want = sum(Fraction(float(t)) for t in terms.ravel())
            assert Fraction(float(got[k, z])) == want, (name, z)
    f["c"][1, 2, 3] = np.nan
    got = Z.plane_sums_exact(f)
    touched = {"c", "c_c", "uz_c", "q_Ex", "q_Ez", "q_q"}
    for k, name in enumerate(Z.PROFILES):
        assert np.isnan(got[k, 1]) == (name in touched) and not np.isnan(got[k, [0, 2, 3]]).any(), name


def test_monitor_exact_against_brute_force(pkg):
    p = pkg.default_params(*TINY)
    f = Z.dyadic_fields(TINY, 6)
    got = Z.monitor_exact(f, p)
    nz = TINY[2]
    cur = lambda w, n1, n2: _fsum(((2.0 * f["c"][n1] - f["c"][n2]) - (2.0 * f["cn"][n1] - f["cn"][n2])) * f["Ez"][w])   # every operation exact
    q = f["c"] - f["cn"]
    want = [cur(nz - 1, nz - 2, nz - 3) * p.K * p.dz * p.dz, cur(0, 1, 2) * p.K * p.dz * p.dz,
            _fsum(4.0 * f["T"][1] - 3.0 * f["T"][0] - f["T"][2]), _fsum(3.0 * f["T"][-1] - 4.0 * f["T"][-2] + f["T"][-3]),
            f["uz"].max(), _fsum(f["ux"] ** 2 + f["uy"] ** 2 + f["uz"] ** 2), _fsum(q), _fsum(q * q), _fsum(f["uz"] * f["T"]),
            np.abs(f["rho"] - p.rho0).max(), 0.0]
    assert got.tolist() == want
    assert got[4] == Z.PLANT_UZ and got[9] == Z.PLANT_RHO
    inner = Z.monitor_exact(f, p, top=False, bottom=False)
    assert inner[:4].tolist() == [0.0] * 4 and inner[4:].tolist() == got[4:].tolist()
    f["c"][2, 1, 1] = np.nan                                                      # plane 2 of 4: both plates read it
    bad = Z.monitor_exact(f, p)
    assert np.isnan(bad[[0, 1, 6, 7]]).all() and bad[10] == 1.0 and np.array_equal(bad[[2, 3, 4, 5, 8, 9]], got[[2, 3, 4, 5, 8, 9]])
    f["c"][2, 1, 1] = 0.0
    f["c"][3, 1, 1] = np.nan                                                      # the upper plate itself: no current reads c there
    bad = Z.monitor_exact(f, p)
    assert np.isnan(bad[[6, 7]]).all() and not np.isnan(bad[[0, 1]]).any() and bad[10] == 1.0


@pytest.mark.parametrize("across", ["x", "y"])
def test_section_ref_is_the_definition_the_other_section_tests_use(pkg, across):
    shape = (131, 70, 3)
    f = Z.random_fields(shape, 9)
    for name in ("uz", "q"):
        v = Z.value(f, name)
        for lo, hi in Z.section_ranges(shape, across).values():
            got = Z.section_ref(pkg, v, across, lo, hi)
            want = TSEC._line_sums(v, across, lo, hi)
            assert got.shape == want.shape and np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (name, lo, hi)
    k = 5
    line = f["uz"][1, k, 3:102] if across == "x" else f["uz"][1, 3:41, k]
    lo, hi = (3, 101) if across == "x" else (3, 40)
    assert Z.section_ref(pkg, f["uz"], across, lo, hi)[1, k] == pkg.section_sum(line)


def test_the_numpy_index_is_ekpnp_hist_bin(pkg):
    f = Z.random_fields((64, 40, 1), 4)
    d = Z.dyadic_fields((64, 40, 4), 4)                                           # values ON bin edges
    for a, b, _ in Z.HIST_SPECS.values():
        for axis in (a, b):
            if axis is None:
                continue
            v = Z.value(f, axis[0]).ravel()
            assert np.array_equal(Z.hist_index(axis, v), pkg.hist_bin(axis[2], axis[3], axis[1], v)), axis
    axis = ("q", 4096, -2.0, 2.0)
    v = np.concatenate([Z.value(d, "q").ravel()[:3000], [np.nan, -2.0, 2.0, 2.0 - 2.0 ** -10]])
    assert np.array_equal(Z.hist_index(axis, v), pkg.hist_bin(-2.0, 2.0, 4096, v))
    counts, nonfinite = Z.hist_counts({"c": v[None, None, :], "cn": np.zeros((1, 1, v.size))}, axis)
    assert counts.sum() == v.size - 1 and nonfinite.tolist() == [1]


def test_rfft2_power_and_its_tolerance_against_the_long_double_transform():
    shape = (20, 12, 2)
    v = Z.dyadic_fields(shape, 8, names=["uz"])["uz"][0]
    exact = TSPEC._exact_power(v)
    tol = Z.power_tolerance(v)
    assert tol == 4.0 * TSPEC._u(v)                                                # the same number as the other file's bound
    assert (np.abs(Z.rfft2_power(v).astype(np.longdouble) - exact) <= tol / 64.0).all()


def test_the_mode_bound_and_the_snapshot_reference_are_the_other_files(pkg):
    v = Z.dyadic_fields(TINY, 2, names=["uz"])["uz"][0]
    assert Z.mode_bound(v) == (v.size + 16) * 2.0 ** -53 * math.fsum(np.abs(v).ravel().tolist())
    ct, st = Z.mode_phase(5, 3, 0, 0)
    assert (ct == 1.0).all() and (st == 0.0).all()
    a = Z.random_fields((6, 4, 5), 1)["T"]
    assert np.array_equal(Z.snapshot_ref(a, (1, 1, 2)), a[::2].astype(np.float32)) and Z.snapshot_ref(a, (2, 2, 1)).shape == (5, 2, 3)
    assert Z.energies(np.array([[[3.0, 4.0], [1.0, 0.0]]])).tolist() == [26.0]
