"""GPU tests of the seeding of x-y structure (csrc/seed.hip; include/ekpnp.h: ekpnp_seed, ekpnp_group_seed).

ekpnp_seed_host is the definition (held against the header's formulas on the CPU, tests/test_seed_cpu.py); the device pass must
leave exactly its bits in the selected field arrays and nothing anywhere else - on every kind of context, however the lattice
is cut, in caller-bound arrays too - and a run started from a device seed must be the run started from get_field, seed_host,
set_field bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
R = (40, 12, 17)   # the suites' run shape
W = (70, 66, 13)   # rows no multiple of 64, 4 620 nodes per plane, slabs of 4 + 4 + 5 planes
SEEDABLE = ["rho", "c", "cn", "ux", "uy", "uz", "T"]
PATTERNS = {"none": (1, 1), "rolls": (3, -2), "squares": (2, 3), "hexagons": (5, 2)}


def _params(pkg, shape, in_place=0):
    p = pkg.default_params(*shape)
    p.pb_iterations = 20
    p.in_place = in_place
    return p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _random_fields(pkg, shape_zyx, seed):
    rng = np.random.default_rng(seed)
    scale = {"rho": 1000.0, "c": 30.0, "cn": 30.0, "phi": 5e-3, "T": 1.0, "Ex": 1e5, "Ey": 1e5, "Ez": 1e5}
    return {n: scale.get(n, 1e-3) * rng.uniform(-1.0, 1.0, size=shape_zyx) for n in pkg.FIELDS}


def _expect(pkg, p, spec, before, z0=0):
    """what every field must be after the seed: seed_host of the selected ones, the others as they were"""
    return {n: pkg.seed_host(p, spec, n, v, z0=z0) if (spec.fields >> pkg.FIELD_ID[n]) & 1 else v for n, v in before.items()}


def _assert_fields(pkg, got, want, tag):
    for n in pkg.FIELDS:
        assert _same(got[n], want[n]), (tag, n, np.argwhere(_bits(got[n]) != _bits(want[n]))[:4])


# ---- 1. the device pass leaves seed_host's bits, and nothing else --------------------------------------------

@pytest.fixture(scope="module")
def started(pkg):
    """one context per shape after initialization(), and its eleven fields (the tests restore the seedable ones from them)"""
    out = {}
    for shape in (R, W):
        s = pkg.Solver(_params(pkg, shape))
        s.initialization()
        out[shape] = (s, s.fields())
    yield out
    for s, _ in out.values():
        s.close()


@pytest.mark.parametrize("relative", [0, 1])
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("shape", [R, W])
def test_seed_equals_seed_host_bit_for_bit(pkg, started, shape, pattern, relative):
    s, f0 = started[shape]
    mx, my = PATTERNS[pattern]
    kw = dict(pattern=pattern, modes=(mx, my), amplitude=1e-2, noise=1e-3, relative=bool(relative), seed=2 ** 40 + 3)
    # seven fields at once
    s.set_fields({n: f0[n] for n in SEEDABLE})
    spec = pkg.seed_spec(fields=SEEDABLE, **kw)
    before = s.fields()
    _assert_fields(pkg, before, f0, "restored")
    s.seed(spec)
    after = s.fields()
    _assert_fields(pkg, after, _expect(pkg, s.p, spec, before), (shape, pattern, relative, "all seven"))
    changed = [n for n in pkg.FIELDS if not _same(after[n], before[n])]
    assert set(changed) <= set(SEEDABLE) and "c" in changed and "rho" in changed, changed
    for n in SEEDABLE:  # the plates keep their boundary values
        assert _same(after[n][0], before[n][0]) and _same(after[n][-1], before[n][-1]), n
    # one field at a time: each call changes its own field only, and the seven calls add up to the one above
    s.set_fields({n: f0[n] for n in SEEDABLE})
    state = s.fields()
    for n in SEEDABLE:
        one = pkg.seed_spec(fields=(n,), **kw)
        s.seed(one)
        state = _expect(pkg, s.p, one, state)
        if n in ("c", "uz"):
            _assert_fields(pkg, s.fields(), state, (shape, pattern, relative, "only " + n))
    _assert_fields(pkg, s.fields(), after, (shape, pattern, relative, "one at a time"))


# ---- 2. however the lattice is held or cut --------------------------------------------------------------

@pytest.fixture(scope="module")
def whole(pkg):
    """random fields of W, a spec with pattern and noise, and the seeded whole lattice (computed once, never modified)"""
    p = _params(pkg, W)
    f = _random_fields(pkg, (W[2], W[1], W[0]), 21)
    spec = pkg.seed_spec(fields=("c", "cn", "uz", "T"), pattern="hexagons", modes=(3, -4), amplitude=2e-2, noise=5e-3, relative=True, seed=12345678901)
    return f, spec, _expect(pkg, p, spec, f)


@pytest.mark.parametrize("in_place", [0, 1])
def test_single_contexts_two_buffer_and_in_place(pkg, whole, in_place):
    f, spec, want = whole
    with pkg.Solver(_params(pkg, W, in_place)) as s:
        s.set_fields(f)
        s.seed(spec)
        _assert_fields(pkg, s.fields(), want, ("in_place", in_place))


def test_stand_alone_slab_contexts_seed_their_own_planes(pkg, whole):
    f, spec, want = whole
    extents = []
    for rank in range(3):
        with pkg.Solver(_params(pkg, W), rank=rank, nranks=3, slab=True) as s:
            z0, nzl = s.z0, s.nz_local
            extents.append((z0, nzl))
            s.set_fields({n: v[z0:z0 + nzl] for n, v in f.items()})
            s.seed(spec)
            _assert_fields(pkg, s.fields(), {n: v[z0:z0 + nzl] for n, v in want.items()}, ("slab", rank))
    assert extents == [(0, 4), (4, 4), (8, 5)]


@pytest.mark.parametrize("nslabs", [2, 3])
def test_groups(pkg, whole, nslabs):
    f, spec, want = whole
    with pkg.Group(_params(pkg, W), nslabs, devices=[0] * nslabs) as g:
        g.set_fields(f)
        g.seed(spec)
        _assert_fields(pkg, g.fields(), want, ("group", nslabs))


# ---- 3. a caller-bound array that is only 8-byte aligned is seeded in place -----------------------------

def test_bound_field_at_an_odd_double_offset(pkg, whole):
    import torch

    f, spec, want = whole
    with pkg.Solver(_params(pkg, W)) as s:
        n = int(np.prod(s.shape))
        pool = torch.zeros(n + 3, dtype=torch.float64, device="cuda")
        off = 1 if pool.data_ptr() % 16 == 0 else 2
        view = pool[off:off + n]
        assert view.data_ptr() % 16 == 8
        s.bind_field("uz", view.data_ptr())
        s.set_fields(f)
        s.seed(spec)
        s.synchronize()
        torch.cuda.synchronize()
        host = pool.cpu().numpy()
        assert _same(host[off:off + n].reshape(s.shape), want["uz"])           # the caller's own memory holds the seeded field
        assert (host[:off] == 0.0).all() and (host[off + n:] == 0.0).all()     # and nothing around it was written
        _assert_fields(pkg, s.fields(), want, "bound uz")


# ---- 4. a run from a device seed is the run from get_field, seed_host, set_field -----------------------

@pytest.mark.parametrize("in_place, lazy", [(0, 1), (0, 0), (1, 1)])
def test_seeded_run_equals_the_host_seeded_twin(pkg, in_place, lazy):
    spec = pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)
    runs = []
    for device_seed in (True, False):
        with pkg.Solver(_params(pkg, R, in_place)) as s:
            s.tune("lazy_efield", lazy)
            s.initialization()
            if device_seed:
                s.seed(spec)
            else:
                for n in ("c", "cn"):
                    s.set_field(n, pkg.seed_host(s.p, spec, n, s.get_field(n)))
            s.fast_Poisson()
            s.init_equilibrium()
            s.step(3)
            runs.append(s.fields())
    _assert_fields(pkg, runs[0], runs[1], ("in_place", in_place, "lazy", lazy))
    c = runs[0]["c"]
    assert np.abs(c - c.mean(axis=(1, 2), keepdims=True)).max() > 1e-4 * np.abs(c).max()  # the run did get its x-y structure


def test_seed_invalidates_the_collides_right_hand_side(pkg):
    """after a step the collide has left the Poisson right-hand side of ITS c, cn behind; a seed must make the next solve re-read
    the arrays: phi after seed + fast_Poisson equals the twin's, whose set_field is known to invalidate"""
    spec = pkg.seed_spec(fields=("c", "cn"), pattern="rolls", modes=(2, 1), amplitude=5e-2, noise=0.0, relative=True, seed=1)
    phis = []
    for device_seed in (True, False):
        with pkg.Solver(_params(pkg, R)) as s:
            s.initialization()
            s.init_equilibrium()
            s.stream_collide_save(0.0)
            if device_seed:
                s.seed(spec)
            else:
                for n in ("c", "cn"):
                    s.set_field(n, pkg.seed_host(s.p, spec, n, s.get_field(n)))
            s.fast_Poisson()
            phis.append(s.get_field("phi"))
    assert _same(phis[0], phis[1])
    assert np.abs(phis[0] - phis[0].mean(axis=(1, 2), keepdims=True)).max() > 0.0
