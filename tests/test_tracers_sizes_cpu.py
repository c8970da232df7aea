"""CPU tests of the tracer cloud past the size thresholds of its kernels (csrc/tracers.hip): what can be held without a device.  The
sizes of tests/_tracers_sizes.py reach the level they are there for, by the constants the source has today; the host definitions the
GPU file (tests/test_tracers_sizes_gpu.py) compares the device with are held against numpy at those sizes; and the cloud and tag-list
builders keep the placements the GPU tests rely on.  Every comparison is of integers or of bit patterns."""
import numpy as np
import pytest

import _tracers_ref as T
import _tracers_sizes as Z


# ---- 0. the sizes and the thresholds ---------------------------------------------------------------------------------------------

def test_the_source_has_the_tile_sizes_the_sizes_were_chosen_for():
    src = Z.source_constants()
    for name, value in Z.CONSTANTS.items():
        assert src.get(name) == value, (name, src.get(name))
    text = open(Z.SOURCE, encoding="utf-8").read()
    assert "constexpr int TR_CHUNK = TR_THREADS * TR_PER_THREAD;" in text
    assert "for (int b0 = 0; b0 < nwg; b0 += 16)" in text          # FINISH_BATCH
    assert "for (unsigned b = 0; b < m; b += TR_THREADS)" in text   # SCAN_TOP_ROUND
    assert (Z.FINISH_BATCH, Z.SCAN_TOP_ROUND) == (16, Z.CONSTANTS["TR_THREADS"])


def test_each_size_crosses_the_threshold_it_is_there_for():
    per_chunk = Z.CONSTANTS["TS_SCAN"] // 256   # runs whose 256 table entries fill one chunk of the scan
    assert per_chunk == 16
    assert {n: Z.levels(n) for n in Z.SORT_NS} == {65536: (16, 16, 1), 65537: (17, 17, 2), 131073: (33, 33, 3), 1048577: (257, 257, 17)}
    for n, (nruns, chunks) in Z.SORT_NS.items():
        assert Z.levels(n)[1:] == (nruns, chunks) and chunks == -(-nruns // per_chunk)
    assert Z.levels(65536)[2] == 1 and 65536 == per_chunk * 4096             # one chunk exactly full ...
    assert 256 * 17 - Z.CONSTANTS["TS_SCAN"] == 256                          # ... and the second holds 256 live entries: 16 live threads of 16
    assert Z.levels(Z.WAVE_N) == (1025, 1025, 65) and Z.levels(Z.WAVE_N - 1)[2] == 64   # one chunk sum more than a wavefront of the top scan holds
    assert [c for _, c in Z.SORT_NS.values()] == [1, 2, 3, 17]
    assert Z.levels(Z.CARRY_N) == (4097, 4097, 257) and Z.levels(Z.CARRY_N)[2] == Z.SCAN_TOP_ROUND + 1   # one live sum in the second round
    assert Z.levels(Z.CARRY_N - 1)[2] == Z.SCAN_TOP_ROUND and Z.CARRY_N <= 1 << 28
    assert {n: Z.levels(n)[0] for n in Z.MOMENT_NS} == Z.MOMENT_NS == {65536: 16, 65537: 17, 131073: 33}
    assert [-(-w // Z.FINISH_BATCH) for w in Z.MOMENT_NS.values()] == [1, 2, 3]   # batches of k_tracers_finish
    assert {n: Z.cell_workgroups(n) for n in Z.CELL_NS} == Z.CELL_NS == {8192: 1, 8193: 2, 24653: 4, 65537: 9}
    cells = [bx * by * bz for bx, by, bz in Z.CELL_GRIDS]
    assert cells == [1, 3072, 8190, 8192, 49152]
    assert [c + 1 <= Z.CONSTANTS["TR_LDS_CELLS"] for c in cells] == [True, True, True, False, False]   # (the lost ones take one counter)
    assert sorted(n % Z.CONSTANTS["TK_IDS"] for n in Z.TRACK_NS[:4]) == [0, 1, 2, 3] and Z.find_workgroups(65537) == 65
    assert [-(-t // Z.CONSTANTS["TR_THREADS"]) for t in Z.TRACK_NTAGS] == [2, 4]   # rounds of the find's LDS fill
    # the byte counts the GPU file asserts, once by hand
    assert Z.cloud_bytes(65537, 17) == 56 * 65537 + 18 * 96 and Z.sort_bytes(65537, 17, 2) == 16 * 65537 + (256 * 17 + 2) * 4 + 4 * 65537


# ---- 1. the host definitions at these sizes --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [65537, 131073])
def test_sort_host_is_the_stable_argsort_of_the_keys(pkg, n):
    shape = Z.SHAPES["T"]
    p = pkg.default_params(*shape)
    x, y, z = Z.special_cloud(shape, n, 300 + n)
    keys = pkg.tracers_sort_key(p, x, y, z)
    assert keys.dtype == np.uint32 and np.array_equal(keys, Z.keys(shape, x, y, z))   # the transcription the GPU file uses
    perm = pkg.tracers_sort_host(p, x, y, z)
    assert perm.dtype == np.int32 and np.array_equal(perm, np.argsort(keys, kind="stable"))
    lost = np.flatnonzero(keys == Z.KEY_LOST)
    assert lost.size >= n // 101 and np.array_equal(perm[n - lost.size:], lost)   # at the end, in their slot order
    assert all(len(set((keys >> (8 * b)) & 255)) > 1 for b in range(4))           # lattice T: every pass moves items


def test_the_clouds_of_the_sort(pkg):
    shape = Z.SHAPES["T"]
    nodes = shape[0] * shape[1] * (shape[2] - 1)
    assert nodes == 73920 > 65536
    p = pkg.default_params(*shape)
    n = 131073
    clouds = Z.sort_clouds(shape, n, 300 + n)
    assert list(clouds) == ["special", "reversed", "one node", "all lost"]
    x, y, z = clouds["special"]
    lost = np.isnan(x)
    assert lost[12] and lost[40::101].all() and all(lost[r * 4096:(r + 1) * 4096].any() for r in range(32))   # lost ones in every full run
    assert np.array_equal(lost, np.isnan(y)) and np.array_equal(lost, np.isnan(z))
    k = Z.keys(shape, *clouds["reversed"]).astype(np.int64)
    assert np.array_equal(k, (n - 1 - np.arange(n)) % nodes) and len(np.unique(k)) == nodes   # every key, most of them twice
    assert len(np.unique(Z.keys(shape, *clouds["one node"]))) == 1
    assert (Z.keys(shape, *clouds["all lost"]) == Z.KEY_LOST).all()
    for name in ("one node", "all lost"):
        assert np.array_equal(pkg.tracers_sort_host(p, *clouds[name]), np.arange(n)), name
    for a in (c for cloud in clouds.values() for c in cloud):
        ok = np.isnan(a) | (a >= 0.0)
        assert ok.all()


def test_the_spread_cloud_hits_several_values_of_every_key_byte(pkg):
    shape = Z.SHAPES["T"]
    p = pkg.default_params(*shape)
    n = 200001   # the generator of the 16 777 217 case at a size the host sorts in a moment
    x, y, z = Z.spread_cloud(shape, n, 5)
    keys = Z.keys(shape, x, y, z)
    assert np.array_equal(keys[:3000], pkg.tracers_sort_key(p, x[:3000], y[:3000], z[:3000]))
    lost = keys == Z.KEY_LOST
    assert n // 128 < lost.sum() < n // 32
    digits = [len(set((keys >> (8 * b)) & 255)) for b in range(4)]
    assert digits[0] == 256 and digits[1] == 256 and digits[2] == 3 and digits[3] == 2, digits   # (0xFF of the lost ones is the third of byte 2)
    alive = keys[~lost].astype(np.int64)
    assert np.abs(np.diff(alive)).min() > 4096 // 2   # neighbours in memory are far apart in the lattice: a sort moves every item
    perm = pkg.tracers_sort_host(p, x, y, z)
    assert np.array_equal(perm, np.argsort(keys, kind="stable"))
    # the full size: the same arithmetic stays inside uint64, checked on the last particles
    i = np.arange(Z.CARRY_N - 4, Z.CARRY_N)
    want = [(int(v) * 2654435761) % 73920 for v in i]
    got = (i.astype(np.uint64) * np.uint64(2654435761)) % np.uint64(73920)
    assert got.tolist() == want and (Z.CARRY_N - 1) * 2654435761 < 1 << 63


# ---- 2. the placements the GPU tests rely on --------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", list(Z.MOMENT_NS))
def test_the_clouds_of_the_moments_keep_their_placement(n):
    shape = Z.SHAPES["R"]
    nz = shape[2]
    nwg = Z.MOMENT_NS[n]
    first = 4096 * (nwg - 1)
    roles = Z.moment_roles(n)
    assert roles == (("lost",) if n == 65536 else Z.MOMENT_ROLES)
    for role in roles:
        x0, y0, z0, where = Z.moments_cloud(shape, n, role, 11)
        lost = np.isnan(x0)
        assert np.array_equal(lost, np.isnan(y0)) and np.array_equal(lost, np.isnan(z0))
        assert where[role] == n - 1 and all(s >= first for k, s in where.items() if k != "second batch")
        want_lost = sorted(s for k, s in where.items() if k in ("lost", "second batch"))
        assert np.flatnonzero(lost).tolist() == want_lost
        if n == 65536:
            assert where == {"lost": n - 1, "z_min": n - 2, "z_max": n - 3}
        else:   # one slot in the last workgroup: slot n - 1 itself
            assert first == n - 1 and set(where) == {role} | ({"second batch"} if n == 131073 else set())
        if n == 131073:
            assert where["second batch"] == 65536 and lost[65536]
        alive = ~lost
        if "z_min" in where:
            assert np.flatnonzero(z0 == z0[alive].min()).tolist() == [where["z_min"]]   # unique
        if "z_max" in where:
            assert np.flatnonzero(z0 == z0[alive].max()).tolist() == [where["z_max"]]
        assert z0[alive].min() >= 0.125 and z0[alive].max() <= nz - 1 - 0.125
        for a, top in ((x0, shape[0]), (y0, shape[1]), (z0, nz - 1)):
            assert np.array_equal((a[alive] * 8.0) % 1.0, np.zeros(alive.sum())) and a[alive].min() >= 0.0 and a[alive].max() < top
        m = Z.moments_exact(n, z0)
        assert m[0] + m[1] == n and m[1] == len(want_lost)
        assert m[8] == z0[alive].sum() and m[9] == (z0[alive] * z0[alive]).sum()   # small dyadic numbers: numpy's sum is exact too
        assert m[9] * 64 < 2 ** 53


def test_the_exact_moments_follow_the_host_advance(pkg):
    """the integer arithmetic of moments_exact against ekpnp_tracers_advance_host on the first and the last particles of the cloud"""
    shape = Z.SHAPES["R"]
    nx, ny, nz = shape
    p = pkg.default_params(*shape)
    p.dx = p.dy = p.dz = 2.0 ** -17
    u = [np.full((nz, ny, nx), Z.MOMENT_U[0]), np.full((nz, ny, nx), Z.MOMENT_U[1]), np.zeros((nz, ny, nx))]
    x0, y0, z0, where = Z.moments_cloud(shape, 65536, "lost", 11)
    pick = np.r_[0:200, 65536 - 200:65536]
    x, y, z, wx, wy = pkg.tracers_advance_host(p, u, x0[pick], y0[pick], z0[pick], h=2.0 ** -10, nsub=Z.MOMENT_NSUB)
    alive = ~np.isnan(x0[pick])
    assert alive.sum() == 399 and np.isnan(x[~alive]).all()
    dx = (x - x0[pick]) + wx * float(nx)
    dy = (y - y0[pick]) + wy * float(ny)
    assert (dx[alive] == 120.0).all() and (dy[alive] == -80.0).all() and T.same(z[alive], z0[pick][alive])
    assert wx[alive].min() >= 1 and wy[alive].max() <= -1   # every particle wraps


@pytest.mark.parametrize("n", list(Z.CELL_NS))
def test_the_cloud_of_the_cell_counts_loses_particles_in_every_workgroup(n):
    x, y, z = Z.cells_cloud(Z.SHAPES["W"], n, 40 + n)
    lost = np.isnan(x)
    assert n // 200 < lost.sum() < n // 50
    assert all(lost[w * 8192:(w + 1) * 8192].any() for w in range(Z.CELL_NS[n] - 1)) and (Z.CELL_NS[n] == 1 or not lost.all())
    for cells in Z.CELL_GRIDS:
        c = T.cell(Z.SHAPES["W"], cells, x, y, z)
        assert np.array_equal(c < 0, lost) and c.max() < cells[0] * cells[1] * cells[2]


# ---- 3. the tag list ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ntags", Z.TRACK_NTAGS)
@pytest.mark.parametrize("n", Z.TRACK_NS)
def test_the_tag_list_is_accepted_and_holds_what_it_must(pkg, n, ntags):
    shape = Z.SHAPES["R"]
    p = pkg.default_params(*shape)
    x, y, z = T.special_cloud(shape, n, 100)
    assert np.isnan(x[Z.TRACK_LOST])
    perm = pkg.tracers_sort_host(p, x, y, z)   # the ids a first sort of this cloud leaves in the slots
    tail = perm[n - n % 4:]
    assert tail.size == n % 4
    ids = Z.tag_list(n, ntags, tail, ntags)
    assert ids.size == ntags and len(set(ids.tolist())) == ntags and ids.min() == 0 and ids.max() == n - 1
    assert np.isin([0, n - 1, Z.TRACK_LOST, *tail], ids).all()
    assert not np.array_equal(ids, np.sort(ids))   # scrambled
    spec = pkg.tracks_spec(ids=ids, values=("T", "q", "uz"))
    assert pkg.tracks_spec_check(p, n, spec).ntags == ntags
    assert [spec.ids[k] for k in range(ntags)] == ids.tolist()


def test_1024_tags_are_accepted_and_1025_refused(pkg):
    p = pkg.default_params(*Z.SHAPES["R"])
    assert pkg.TRACERS_MAX_TRACKS == 1024
    spec = pkg.tracks_spec(ids=Z.tag_list(65537, 1024, (), 1))
    assert pkg.tracks_spec_check(p, 65537, spec).ntags == 1024
    more = pkg.tracks_spec(ids=np.arange(1025))
    assert more.ntags == 1025
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.tracks_spec_check(p, 65537, more)
    assert "ntags = 1025" in str(e.value) and "status 1" in str(e.value)
