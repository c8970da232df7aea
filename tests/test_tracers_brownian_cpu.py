"""CPU tests of the Brownian tracers (csrc/tracers.hip; include/ekpnp.h: ekpnp_tracers_kick, ekpnp_tracers_advance_brownian_host): the
host-only entry points, which ARE the definitions the device is held against in tests/test_tracers_brownian_gpu.py.  No device is
needed.

The draw and the advance are compared with a numpy transcription of the header's text (tests/_tracers_brownian_ref.py) on the float64
BIT PATTERN.  The statistical checks have bounds that come from the sampling error of their own estimators - five standard
deviations, or the 1 - 10^-6 quantile of a chi-square - and fixed seeds, so they are deterministic."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _tracers_brownian_ref as B
import _tracers_ref as T

W = (70, 66, 13)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ["ekpnp_tracers_kick", "ekpnp_tracers_advance_brownian_host", "ekpnp_tracers_advance_brownian", "ekpnp_tracers_epoch"]
EDGE = [0, 1, 2 ** 31 - 1, 2 ** 32, 2 ** 40]


# ---- 1. the interface ------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_mirrored(pkg):
    lib = pkg.load_library()
    for name in NAMES:
        assert name in pkg.exported_symbols()
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    assert not [n for n in pkg.exported_symbols() if n.startswith("ekpnp_group_tracers")]
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ekpnp.h")).read())
    for decl in ("void ekpnp_tracers_kick(uint64_t seed, int64_t id, int64_t epoch, double r[3]);",
                 "int32_t* wy, double mu, double D, double h, int nsub, uint64_t seed, int64_t epoch);",
                 "int ekpnp_tracers_advance_brownian(ekpnp_ctx* ctx, double mu, double D, double h, int nsub, uint64_t seed);",
                 "int ekpnp_tracers_epoch(ekpnp_ctx* ctx, int64_t* epoch);"):
        assert decl in hdr, decl
    assert lib.ekpnp_tracers_kick.restype is None and len(lib.ekpnp_tracers_kick.argtypes) == 4
    assert len(lib.ekpnp_tracers_advance_brownian_host.argtypes) == 20 and len(lib.ekpnp_tracers_advance_brownian.argtypes) == 6
    assert lib.ekpnp_tracers_advance_brownian.argtypes[5] is C.c_uint64 and lib.ekpnp_tracers_advance_brownian_host.argtypes[19] is C.c_int64
    # the structures of the cloud are what they were
    assert C.sizeof(pkg.TracersSpec) == 80 and C.sizeof(pkg.TracksSpec) == 4152
    assert [getattr(pkg.TracersSpec, n).offset for n in ("n", "mode", "gx", "gy", "gz", "seed", "lo", "hi")] == [0, 8, 12, 16, 20, 24, 32, 56]
    for m in ("tracers_advance", "tracers_epoch"):
        assert hasattr(pkg.Solver, m), m
    for f in ("tracers_kick", "tracers_advance_brownian_host"):
        assert callable(getattr(pkg, f)), f
    assert not [m for m in dir(pkg.Group) if "tracers" in m]


def test_refusals_give_the_offending_number(pkg):
    L = pkg.load_library()
    p = pkg.default_params(*W)
    a = np.full(10, 2.5)
    w = np.zeros(10, dtype=np.int32)
    u = np.zeros((W[2], W[1], W[0]))
    ptr = lambda v: v.ctypes.data_as(C.c_void_p)
    #        0           1       2       3       4     5     6     7   8     9       10      11      12      13      14   15    16     17 18 19
    args = [C.byref(p), ptr(u), ptr(u), ptr(u), None, None, None, 10, None, ptr(a), ptr(a), ptr(a), ptr(w), ptr(w), 0.0, 0.5, 0.25, 1, 7, 0]
    assert L.ekpnp_tracers_advance_brownian_host(*args) == 0   # mu == 0: the E arrays are not needed; ids NULL: 0 .. n-1
    cases = [(15, -1.5, b"D = -1.5"), (15, math.nan, b"D = nan"), (15, math.inf, b"D = inf"), (16, -0.25, b"D*h = -0.125"),
             (17, 0, b"nsub = 0"), (17, -2, b"nsub = -2"), (17, 4097, b"nsub = 4097"), (14, math.inf, b"mu = inf"), (16, math.nan, b"h = nan"),
             (16, math.inf, b"h = inf"), (19, -3, b"epoch = -3"), (7, -1, b"n = -1"), (7, (1 << 28) + 1, b"n = 268435457"), (14, 1e-8, b"NULL")]
    for k, v, msg in cases:
        bad = list(args)
        bad[k] = v
        assert L.ekpnp_tracers_advance_brownian_host(*bad) == 1 and msg in L.ekpnp_last_error(None), (k, v, L.ekpnp_last_error(None))
    for k in (0, 1, 9, 13):
        bad = list(args)
        bad[k] = None
        assert L.ekpnp_tracers_advance_brownian_host(*bad) == 1 and b"NULL" in L.ekpnp_last_error(None), k
    thin = pkg.default_params(8, 8, 8)
    thin.nz = 2
    bad = list(args)
    bad[0] = C.byref(thin)
    assert L.ekpnp_tracers_advance_brownian_host(*bad) == 1 and b"nz = 2" in L.ekpnp_last_error(None)
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.tracers_advance_brownian_host(p, [u, u, u], a, a, a, D=-2.0, h=1e-3)
    assert "D = -2" in str(e.value) and "status 1" in str(e.value)
    L.ekpnp_tracers_kick(1, 2, 3, None)   # a NULL r is not dereferenced
    for name in ("advance_brownian", "epoch"):
        assert getattr(L, "ekpnp_tracers_" + name)(None, *([0.0, 0.0, 0.0, 1, 0] if name == "advance_brownian" else [None])) == 1


# ---- 2. the draw -------------------------------------------------------------------------------------------------------

def test_kick_equals_the_numpy_philox_exactly(pkg):
    for seed in (0, 1, 2 ** 63 + 11, 2 ** 64 - 1):
        for epoch in EDGE:
            want = B.kick(seed, EDGE, epoch)
            got = np.stack([pkg.tracers_kick(seed, i, epoch) for i in EDGE], axis=1)
            assert T.same(got, want), (seed, epoch)
    r = np.stack([pkg.tracers_kick(5, i, 9) for i in range(4096)])
    assert r.shape == (4096, 3) and (np.abs(r) < 1.0).all() and (r != 0.0).all()
    assert np.array_equal(r * 2.0 ** 31 - 0.5, np.round(r * 2.0 ** 31 - 0.5))   # (int32 + 0.5) * 2^-31: exact
    assert abs(r.mean()) < 5.0 / math.sqrt(3.0 * r.size) and abs((r * r).mean() - 1.0 / 3.0) < 5.0 * math.sqrt(4.0 / 45.0 / r.size)
    # the same id, seed and epoch repeat; any of the three, and the axis, change the number
    base = pkg.tracers_kick(5, 7, 9)
    assert T.same(base, pkg.tracers_kick(5, 7, 9)) and len(set(base)) == 3
    for other in ((6, 7, 9), (5, 8, 9), (5, 7, 10), (5, 7, 9 + 2 ** 32), (5, 7 + 2 ** 32, 9), (5 + 2 ** 32, 7, 9)):
        assert not (pkg.tracers_kick(*other) == base).any(), other
    assert T.same(pkg.tracers_kick(5, 7, 9), B.kick(5, [7], 9)[:, 0])


def test_no_counter_of_a_kick_is_a_counter_of_seed_uniform():
    """seed_uniform's counter is {node low, node high, field, 0}; a kick's fourth word has bit 31 set whatever the id"""
    for i in EDGE + [2 ** 28 - 1, 2 ** 62]:
        assert (B.KICK_TAG | (i >> 32)) & 0xFFFFFFFF != 0
    assert B.KICK_TAG == 0x80000000


# ---- 3. the advance against its transcription --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def w_case(pkg):
    p = pkg.default_params(*W)
    u, E = T.random_fields(W, 71, T.U_SCALE, T.E_SCALE)
    u[1][5, 7, 9] = np.nan                         # a NaN node: the particles whose stencil holds it are lost
    x, y, z = B.plate_cloud(W, 1000, 72)
    x[40], y[40], z[40] = 8.5, 6.5, 4.5            # ... this one from the first evaluation on
    for a in (*u, *E, x, y, z):
        a.setflags(write=False)
    return p, u, E, x, y, z


@pytest.mark.parametrize("mu", [0.0, T.MU, -T.MU])
def test_advance_brownian_host_equals_the_transcription_bit_for_bit(pkg, w_case, mu):
    p, u, E, x, y, z = w_case
    h, D = T.substep(p), B.diffusivity(p)
    kw = dict(E=E, mu=mu, D=D, h=h, nsub=7, seed=B.SEED, epoch=2 ** 32 - 3)   # the epoch's low word wraps inside the call
    got = pkg.tracers_advance_brownian_host(p, u, x, y, z, **kw)
    want = B.advance(p, u, x, y, z, **kw)
    for k, name in enumerate(("x", "y", "z")):
        assert T.same(got[k], want[k]), (name, np.flatnonzero(T.bits(got[k]) != T.bits(want[k]))[:5])
    assert np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4])
    gx, gy, gz, wx, wy = got
    lost = np.isnan(gx)
    assert np.array_equal(lost, np.isnan(gy)) and np.array_equal(lost, np.isnan(gz))
    assert lost[12] and lost[40] and 2 <= lost.sum() < 100   # lost from the start, the NaN node's, and a few that met it on their way
    alive = ~lost
    assert (gx[alive] >= 0).all() and (gx[alive] < W[0]).all() and (gy[alive] >= 0).all() and (gy[alive] < W[1]).all()
    assert (gz[alive] >= 0).all() and (gz[alive] <= W[2] - 1).all()
    assert (wx > 0).any() and (wx < 0).any() and (wy > 0).any() and (wy < 0).any()   # wraps either way
    # the noise matters, and so does the mobility
    plain = pkg.tracers_advance_host(p, u, x, y, z, E=E, mu=mu, h=h, nsub=7)
    both = alive & ~np.isnan(plain[0])
    assert (gx[both] != plain[0][both]).all() and (gz[both] != plain[2][both]).mean() > 0.9
    if mu != 0.0:
        assert not T.same(pkg.tracers_advance_brownian_host(p, u, x, y, z, **dict(kw, mu=0.0))[0], gx)


def test_reflection_at_both_plates_happened_and_is_a_reflection(pkg, w_case):
    """one substep without a flow: the particles near a plate that are kicked through it come back by what they overshot"""
    p, u, E, x, y, z = w_case
    zero = [np.zeros_like(u[0])] * 3
    h, D = T.substep(p), B.diffusivity(p)
    kz = B.kick_lengths(p, D, h)[2]
    got = pkg.tracers_advance_brownian_host(p, zero, x, y, z, D=D, h=h, nsub=1, seed=B.SEED, epoch=4)
    r = B.kick(B.SEED, np.arange(1000), 4)
    raw = z + kz * r[2]
    top = float(W[2] - 1)
    alive = ~np.isnan(z)
    low, high = alive & (raw < 0.0), alive & (raw > top)
    assert low.sum() >= 10 and high.sum() >= 10
    assert T.same(got[2][low], 0.0 - raw[low]) and T.same(got[2][high], top - (raw[high] - top))
    inside = alive & ~low & ~high
    assert T.same(got[2][inside], raw[inside]) and (got[2][alive] > 0.0).all() and (got[2][alive] < top).all()   # nobody sticks to a plate
    # a kick longer than the channel (up to 5 cells between plates 2 apart): reflected once or twice, then held by a plate
    thin = pkg.default_params(8, 8, 8)
    thin.nz = 3
    Dk = (5.0 * thin.dz) ** 2 / (6.0 * 1e-3)
    k = B.kick_lengths(thin, Dk, 1e-3)[2]
    uz = [np.zeros((3, 8, 8))] * 3
    raw = 1.0 + k * B.kick(1, np.arange(256), 0)[2]
    want, ok = B._reflect_z(raw, 2.0)
    out = pkg.tracers_advance_brownian_host(thin, uz, np.full(256, 4.0), np.full(256, 4.0), np.full(256, 1.0), D=Dk, h=1e-3, seed=1)
    assert ok.all() and T.same(out[2], want) and (out[2] >= 0.0).all() and (out[2] <= 2.0).all()
    assert (raw > 4.0).sum() > 10 and (out[2][raw > 4.0] == 0.0).all()   # through the top by more than the channel: held at the bottom
    assert (raw < -2.0).sum() > 10 and (out[2][raw < -2.0] < 2.0).all()  # reflected at the bottom, then at the top


# ---- 4. the structure of the draws -------------------------------------------------------------------------------------

def test_equal_positions_and_different_ids_separate_and_equal_ids_repeat(pkg, w_case):
    p, u, E, x, y, z = w_case
    h, D = T.substep(p), B.diffusivity(p)
    n = 64
    same = [np.full(n, 20.25), np.full(n, 30.5), np.full(n, 6.75)]
    a = pkg.tracers_advance_brownian_host(p, u, *same, D=D, h=h, nsub=1, seed=3)
    for k in range(3):
        assert len(set(a[k])) == n, k                        # every id its own numbers
    b = pkg.tracers_advance_brownian_host(p, u, *same, D=D, h=h, nsub=1, seed=3, ids=np.full(n, 17))
    for k in range(3):
        assert len(set(b[k])) == 1 and b[k][0] == a[k][17]  # one id, one path
    c = pkg.tracers_advance_brownian_host(p, u, *same, D=D, h=h, nsub=1, seed=3)
    assert all(T.same(a[k], c[k]) for k in range(3))         # and the same call repeats
    d = pkg.tracers_advance_brownian_host(p, u, *same, D=D, h=h, nsub=1, seed=4)
    e = pkg.tracers_advance_brownian_host(p, u, *same, D=D, h=h, nsub=1, seed=3, epoch=1)
    assert (d[0] != a[0]).all() and (e[0] != a[0]).all()


def test_one_call_of_seven_equals_seven_calls_of_one_with_the_epochs_in_a_row(pkg, w_case):
    p, u, E, x, y, z = w_case
    h, D = T.substep(p), B.diffusivity(p)
    e0 = 2 ** 40 - 2
    whole = pkg.tracers_advance_brownian_host(p, u, x, y, z, E=E, mu=T.MU, D=D, h=h, nsub=7, seed=B.SEED, epoch=e0)
    s = (x, y, z, None, None)
    for it in range(7):
        s = pkg.tracers_advance_brownian_host(p, u, *s, E=E, mu=T.MU, D=D, h=h, nsub=1, seed=B.SEED, epoch=e0 + it)
    for k in range(3):
        assert T.same(whole[k], s[k])
    assert np.array_equal(whole[3], s[3]) and np.array_equal(whole[4], s[4])
    shifted = pkg.tracers_advance_brownian_host(p, u, x, y, z, E=E, mu=T.MU, D=D, h=h, nsub=7, seed=B.SEED, epoch=e0 + 1)
    assert not T.same(shifted[0], whole[0])


def test_an_ids_permutation_gives_the_permuted_result(pkg, w_case):
    p, u, E, x, y, z = w_case
    h, D = T.substep(p), B.diffusivity(p)
    kw = dict(E=E, mu=T.MU, D=D, h=h, nsub=7, seed=B.SEED, epoch=5)
    straight = pkg.tracers_advance_brownian_host(p, u, x, y, z, **kw)
    perm = np.random.default_rng(3).permutation(1000).astype(np.int32)
    moved = pkg.tracers_advance_brownian_host(p, u, x[perm], y[perm], z[perm], ids=perm, **kw)   # slot s holds particle perm[s]
    for k in range(3):
        assert T.same(moved[k], straight[k][perm]), k
    assert np.array_equal(moved[3], straight[3][perm]) and np.array_equal(moved[4], straight[4][perm])
    by_slot = pkg.tracers_advance_brownian_host(p, u, x[perm], y[perm], z[perm], **kw)           # keyed by slot: other paths
    assert not T.same(by_slot[0], moved[0])


@pytest.mark.parametrize("mu", [0.0, T.MU])
def test_no_diffusivity_gives_the_numbers_of_advance_host(pkg, w_case, mu):
    p, u, E, x, y, z = w_case
    for h in (T.substep(p), -T.substep(p)):   # D == 0 runs backwards too
        got = pkg.tracers_advance_brownian_host(p, u, x, y, z, E=E, mu=mu, D=0.0, h=h, nsub=7, seed=B.SEED, epoch=11)
        want = pkg.tracers_advance_host(p, u, x, y, z, E=E, mu=mu, h=h, nsub=7)
        for k in range(5):
            assert np.array_equal(got[k], want[k], equal_nan=True), (h, k)


# ---- 5. statistics -----------------------------------------------------------------------------------------------------

def test_free_diffusion_has_the_variance_of_the_gaussian_it_replaces(pkg):
    """u = 0, E = 0: K independent uniform kicks of variance kx^2/3 each.  The sample variance of n displacements has the relative
    standard deviation sqrt(2/n) (the sum of 64 uniforms is Gaussian to that accuracy: its excess kurtosis is -1.2/64), the sample
    mean sqrt(K kx^2/3/n)."""
    shape = (16, 12, 9)
    p = pkg.default_params(*shape)
    n, K = 65536, 64
    zero = [np.zeros((shape[2], shape[1], shape[0]))] * 3
    spec = pkg.tracers_spec(n=n, p=p, seed=2)
    x0, y0, z0 = pkg.tracers_seed_host(p, spec)
    h = 1e-3
    for seed, cells in ((1, 0.75), (2 ** 63 + 5, 3.0)):
        D = (cells * p.dx) ** 2 / (6.0 * h)
        kx, ky, _ = B.kick_lengths(p, D, h)
        x, y, z, wx, wy = pkg.tracers_advance_brownian_host(p, zero, x0, y0, z0, D=D, h=h, nsub=K, seed=seed)
        assert not np.isnan(x).any()
        for name, d, k in (("x", (x - x0) + wx * float(shape[0]), kx), ("y", (y - y0) + wy * float(shape[1]), ky)):
            var = K * k * k / 3.0
            rel = (d * d).mean() / var - 1.0
            print(f"seed {seed} {name}: <d^2> / (K k^2/3) - 1 = {rel:+.2e} (bound {5.0 * math.sqrt(2.0 / n):.2e}), <d> = {d.mean():+.2e} (bound {5.0 * math.sqrt(var / n):.2e})")
            assert abs(rel) <= 5.0 * math.sqrt(2.0 / n), (seed, name, rel)
            assert abs(d.mean()) <= 5.0 * math.sqrt(var / n), (seed, name, d.mean())
        assert abs(np.corrcoef((x - x0) + wx * 16.0, (y - y0) + wy * 12.0)[0, 1]) < 5.0 / math.sqrt(n)   # the axes draw independent numbers


def _chi2_sf7(x):
    """the survival function of a chi-square with seven degrees of freedom (closed form for odd degrees)"""
    return math.erfc(math.sqrt(x / 2.0)) + math.sqrt(2.0 * x / math.pi) * math.exp(-x / 2.0) * (1.0 + x / 3.0 + x * x / 15.0)


def test_reflection_keeps_a_uniform_cloud_uniform(pkg):
    """without a flow the folded, reflected walk preserves the uniform density exactly; the particles are independent, so the
    counts of eight equal cells are multinomial and their chi-square has seven degrees of freedom"""
    shape = (8, 8, 9)
    p = pkg.default_params(*shape)
    n, h = 65536, 1e-3
    zero = [np.zeros((shape[2], shape[1], shape[0]))] * 3
    x0, y0, z0 = pkg.tracers_seed_host(p, pkg.tracers_spec(n=n, box=((0, 8), (0, 8), (0, 8)), seed=6))
    D = (1.5 * p.dz) ** 2 / (6.0 * h)
    assert abs(B.kick_lengths(p, D, h)[2] - 1.5) < 1e-12
    lo, hi = 20.0, 80.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _chi2_sf7(mid) > 1e-6 else (lo, mid)
    assert 40.0 < hi < 45.0   # the 1 - 10^-6 quantile of chi-square(7)
    x, y, z, _, _ = pkg.tracers_advance_brownian_host(p, zero, x0, y0, z0, D=D, h=h, nsub=32, seed=12)
    assert not np.isnan(z).any() and z.min() > 0.0 and z.max() < 8.0
    counts = np.bincount(np.minimum(z.astype(np.int64), 7), minlength=8)
    chi2 = float(((counts - n / 8.0) ** 2 / (n / 8.0)).sum())
    print(f"counts {counts.tolist()}, chi2 {chi2:.2f} (quantile {hi:.2f})")
    assert chi2 < hi
    assert np.abs(z - z0).mean() > 1.0   # and it did move: a clamped walk would have piled thousands onto the plates


def test_a_mobile_diffusing_cloud_relaxes_to_the_boltzmann_profile(pkg):
    """uniform Ez, u = 0: the drift mu Ez against the diffusion D gives the density exp(z / l) between the plates, l = D / (mu Ez dz)
    cells - the Boltzmann profile of an ion whose mobility and diffusivity obey the Einstein relation.  The cloud starts uniform.
    At this step (kz = 0.1 l) the mean comes out 3.0716 against 3.0746: -0.23 sigma; the scheme's first-order bias does not show."""
    shape = (4, 4, 5)
    top = 4.0
    p = pkg.default_params(*shape)
    n, ell, kz, h = 4096, 1.0, 0.1, 1e-3
    D = (kz * p.dz) ** 2 / (6.0 * h)
    Ez, mu = 1e5, D / (ell * 1e5 * p.dz)
    assert abs(B.kick_lengths(p, D, h)[2] - kz) < 1e-12 and kz <= 0.1 * ell and abs(D / (mu * Ez * p.dz) - ell) < 1e-12
    zero = np.zeros((shape[2], shape[1], shape[0]))
    E = [zero, zero, np.full_like(zero, Ez)]
    x0, y0, z0 = pkg.tracers_seed_host(p, pkg.tracers_spec(n=n, box=((0, 4), (0, 4), (0, 4)), seed=8))
    s = (x0, y0, z0, None, None)
    steps = 0
    # 8192 substeps.  Per substep the drift is v = kz^2 / (6 l) cells and the diffusivity d = kz^2 / 6 cells^2; the slowest mode of the
    # reflected drift-diffusion decays at v^2 / (4 d) + pi^2 d / top^2 = 1.4e-3 per substep: what is left of the start is e^-11 of it
    for _ in range(2):
        s = pkg.tracers_advance_brownian_host(p, [zero] * 3, *s, E=E, mu=mu, D=D, h=h, nsub=4096, seed=21, epoch=steps)
        steps += 4096
    z = s[2]
    assert not np.isnan(z).any()
    # the truncated exponential on [0, top] with density exp(z / l): its mean and variance
    a = top / ell
    mean = top / (1.0 - math.exp(-a)) - ell
    var = ell * ell - top * top * math.exp(-a) / (1.0 - math.exp(-a)) ** 2
    sigma = math.sqrt(var / n)
    print(f"mean z {z.mean():.4f}, analytic {mean:.4f}, deviation {(z.mean() - mean) / sigma:+.2f} sigma (sigma {sigma:.4f}); start {z0.mean():.4f}")
    assert abs(z0.mean() - mean) > 20.0 * sigma   # the start is far from it
    assert abs(z.mean() - mean) <= 5.0 * sigma
