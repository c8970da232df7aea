"""CPU-side checks of the seeding of x-y structure (include/ekpnp.h: ekpnp_seed_spec_check, ekpnp_seed_uniform, ekpnp_seed_host,
ekpnp_seed, ekpnp_group_seed; `ekpnp_main --seed-pattern`).  No device needed.

ekpnp_seed_host is THE definition of a seed; here it is held against the formulas of the header written out in Python:
  - the noise against a numpy Philox4x32-10 that first reproduces the generator's published known answers, with == on doubles;
  - the seeded planes within 2**-40 (|A| + |B|) max(1, |v|) per node.  A wrong index, phase, envelope or pattern shows at order A,
    two libms' cos / sin differ below 2**-50: the bound sits between the two.  With A = 0 the result equals the model exactly."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
INVALID = 1  # EKPNP_ERR_INVALID
W = (70, 66, 13)  # rows that are no multiple of 64, 4 620 nodes per plane, slabs of 4 + 4 + 5 planes
SEEDABLE = ["rho", "c", "cn", "ux", "uy", "uz", "T"]
ENTRY_POINTS = ["ekpnp_seed_spec_check", "ekpnp_seed_uniform", "ekpnp_seed_host", "ekpnp_seed", "ekpnp_group_seed"]

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """numpy Philox4x32-10 on arrays of counters [..., 4] and keys [..., 2] (uint64 arithmetic on 32-bit words)"""
    c = [np.asarray(ctr[..., k], dtype=np.uint64) for k in range(4)]
    k0, k1 = (np.asarray(key[..., k], dtype=np.uint64) for k in range(2))
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return np.stack(c, axis=-1)


def uniform_model(seed, node, field_id):
    """r of the header: counter (node lo, node hi, field, 0), key (seed lo, seed hi), 53 bits of w0, w1, exact in [-1, 1)"""
    node = np.asarray(node, dtype=np.uint64)
    seed = np.broadcast_to(np.asarray(seed, dtype=np.uint64), node.shape)
    fid = np.broadcast_to(np.asarray(field_id, dtype=np.uint64), node.shape)
    mask = np.uint64(0xFFFFFFFF)
    ctr = np.stack([node & mask, node >> np.uint64(32), fid, np.zeros_like(node)], axis=-1)
    key = np.stack([seed & mask, seed >> np.uint64(32)], axis=-1)
    w = philox4x32_10(ctr, key)
    k = (w[..., 0] >> np.uint64(5)) * np.uint64(1 << 26) + (w[..., 1] >> np.uint64(6))
    return k.astype(np.float64) * 2.0 ** -52 - 1.0


def tables_model(p, mx, my):
    """cX, sX, cY, sY, c2Y, env of the header; math.cos / math.sin are the C library's"""
    nx, ny, nz = p.nx, p.ny, p.nz
    cX = np.array([math.cos(2.0 * math.pi * float((mx * x) % nx) / float(nx)) for x in range(nx)])
    sX = np.array([math.sin(2.0 * math.pi * float((mx * x) % nx) / float(nx)) for x in range(nx)])
    cY = np.array([math.cos(2.0 * math.pi * float((my * y) % ny) / float(ny)) for y in range(ny)])
    sY = np.array([math.sin(2.0 * math.pi * float((my * y) % ny) / float(ny)) for y in range(ny)])
    c2Y = np.array([math.cos(2.0 * math.pi * float((2 * my * y) % ny) / float(ny)) for y in range(ny)])
    env = np.array([math.sin(math.pi * float(z) / float(nz - 1)) for z in range(nz)])
    return cX, sX, cY, sY, c2Y, env


def seed_model(p, spec, field_id, v, z0=0):
    """the definition in numpy: every operation rounded once (numpy never fuses), plates untouched"""
    nx, ny, nz = p.nx, p.ny, p.nz
    cX, sX, cY, sY, c2Y, env = tables_model(p, spec.mx, spec.my)
    cXg, sXg, cYg, sYg, c2Yg = cX[None, :], sX[None, :], cY[:, None], sY[:, None], c2Y[:, None]
    if spec.pattern == 0:
        h = np.zeros((ny, nx))
    elif spec.pattern == 1:
        h = cXg * cYg - sXg * sYg
    elif spec.pattern == 2:
        h = cXg * cYg
    else:
        h = (2.0 * (cXg * cYg) + c2Yg) / 3.0
    out = np.array(v, dtype=np.float64, copy=True)
    for zl in range(out.shape[0]):
        z = z0 + zl
        if z < 1 or z > nz - 2:
            continue
        node = (np.uint64(z) * np.uint64(ny) + np.arange(ny, dtype=np.uint64)[:, None]) * np.uint64(nx) + np.arange(nx, dtype=np.uint64)[None, :]
        r = uniform_model(spec.seed, node, field_id)
        pp = spec.amplitude * h
        q = spec.noise * r
        t = pp + q
        s = env[z] * t
        out[zl] = out[zl] + out[zl] * s if spec.relative else out[zl] + s
    return out


def _header_code():
    txt = open(os.path.join(ROOT, "include", "ekpnp.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only, comments stripped


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_entry_points_are_declared_exported_and_mirrored(pkg):
    code = _header_code()
    lib = pkg.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|double)\s+%s\s*\(" % name, code), f"include/ekpnp.h does not declare {name}"
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert name in pkg.exported_symbols()
        assert getattr(lib, name).argtypes is not None, f"solver.py gives {name} no signature"
    assert re.search(r"EKPNP_SEED_NONE\s*=\s*0,\s*EKPNP_SEED_ROLLS\s*=\s*1,\s*EKPNP_SEED_SQUARES\s*=\s*2,\s*EKPNP_SEED_HEXAGONS\s*=\s*3", code)
    assert C.sizeof(pkg.SeedSpec) == 48
    assert [n for n, _ in pkg.SeedSpec._fields_] == ["fields", "pattern", "mx", "my", "relative", "reserved", "seed", "amplitude", "noise"]
    assert (pkg.SeedSpec.seed.offset, pkg.SeedSpec.amplitude.offset, pkg.SeedSpec.noise.offset) == (24, 32, 40)
    for name in ("seed_spec", "seed_uniform", "seed_host", "SeedSpec"):
        assert hasattr(pkg, name), name
    for cls in (pkg.Solver, pkg.Group):
        assert hasattr(cls, "seed"), cls.__name__
    s = pkg.seed_spec(fields=("c", "T"), pattern="hexagons", modes=(2, -1), amplitude=0.5, noise=0.25, relative=False, seed=9)
    assert (s.fields, s.pattern, s.mx, s.my, s.relative, s.reserved, s.seed, s.amplitude, s.noise) == ((1 << 1) | (1 << 10), 3, 2, -1, 0, 0, 9, 0.5, 0.25)


def test_the_numpy_philox_reproduces_the_published_known_answers():
    """Random123's kat_vectors for philox4x32-10: zero, all-ones and the digits of pi"""
    kat = [
        ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
        ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
        ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
    ]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert [int(x) for x in got] == want, ([hex(int(x)) for x in got], [hex(x) for x in want])


def test_seed_uniform_equals_the_numpy_philox_exactly(pkg):
    rng = np.random.default_rng(11)
    seeds = np.concatenate([np.array([0, 1, 7, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 12345], dtype=np.uint64), rng.integers(0, 2 ** 63, size=6, dtype=np.uint64)])
    nodes = np.concatenate([np.array([0, 1, 2, 3, 4, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 + 17, 2 ** 64 - 1], dtype=np.uint64),
                            rng.integers(0, 2 ** 63, size=9, dtype=np.uint64)])
    assert seeds.dtype == np.uint64 and nodes.dtype == np.uint64 and int(nodes[10]) == 2 ** 64 - 1
    n = 0
    for fid in (1, 2, 6, 10):
        for seed in seeds:
            want = uniform_model(seed, nodes, fid)
            got = np.array([pkg.seed_uniform(int(seed), int(node), fid) for node in nodes])
            assert (got == want).all(), (int(seed), fid, got, want)
            assert ((got >= -1.0) & (got < 1.0)).all()
            n += len(nodes)
    assert n >= 300
    got = [pkg.seed_uniform(7, node, "c") for node in range(5)]
    assert [round(r, 8) for r in got] == [-0.00992042, 0.77469325, -0.42072669, -0.49351049, -0.71532853]


@pytest.fixture(scope="module")
def base(pkg):
    """the fields of W the seeds below start from (never modified): values of the usual magnitudes, some of them negative"""
    p = pkg.default_params(*W)
    rng = np.random.default_rng(5)
    scale = {"rho": 1000.0, "c": 30.0, "cn": 30.0, "T": 1.0}
    v = {n: scale.get(n, 1e-3) * rng.uniform(-1.0, 1.0, size=(W[2], W[1], W[0])) for n in SEEDABLE}
    return p, v


@pytest.mark.parametrize("relative", [0, 1])
@pytest.mark.parametrize("pattern, modes", [("none", (1, 1)), ("rolls", (3, -2)), ("squares", (2, 3)), ("hexagons", (5, 7))])
def test_seed_host_against_the_formulas_in_numpy(pkg, base, pattern, modes, relative):
    p, v = base
    A, B = 0.125, 0.03
    spec = pkg.seed_spec(fields=("c", "uz"), pattern=pattern, modes=modes, amplitude=A, noise=B, relative=bool(relative), seed=2 ** 33 + 5)
    for name in ("c", "uz", "T"):  # (the field need not be selected by spec.fields: the caller chooses)
        fid = pkg.FIELD_ID[name]
        got = pkg.seed_host(p, spec, name, v[name])
        want = seed_model(p, spec, fid, v[name])
        bound = 2.0 ** -40 * (abs(A) + abs(B)) * np.maximum(1.0, np.abs(v[name]))
        err = np.abs(got - want)
        print(f"{pattern} relative {relative} {name}: largest |lib - numpy| / bound = {(err / bound).max():.3e}")
        assert (err <= bound).all(), (pattern, relative, name, float((err / bound).max()))
        # the plates are bitwise untouched, the interior has moved at order A
        assert (_bits(got[0]) == _bits(v[name][0])).all() and (_bits(got[-1]) == _bits(v[name][-1])).all()
        assert np.abs(got[1:-1] - v[name][1:-1]).max() > 1e-4 * (np.abs(v[name]).max() if relative else 1.0)
    # A = 0: noise alone, equal to the model exactly
    spec0 = pkg.seed_spec(fields=("c",), pattern=pattern, modes=modes, amplitude=0.0, noise=B, relative=bool(relative), seed=3)
    got, want = pkg.seed_host(p, spec0, "c", v["c"]), seed_model(p, spec0, pkg.FIELD_ID["c"], v["c"])
    assert (got == want).all()


def test_seed_host_leaves_its_input_and_every_other_array_alone_and_cuts_into_pieces(pkg, base):
    p, v = base
    keep = {n: a.copy() for n, a in v.items()}
    spec = pkg.seed_spec(fields=("cn",), pattern="squares", modes=(2, 3), amplitude=1e-2, noise=1e-3, relative=True, seed=77)
    whole = pkg.seed_host(p, spec, "cn", v["cn"])
    for n in SEEDABLE:  # seed_host works on a copy; nothing else is touched
        assert (_bits(v[n]) == _bits(keep[n])).all(), n
    pieces = [pkg.seed_host(p, spec, "cn", v["cn"][a:b], z0=a) for a, b in ((0, 4), (4, 8), (8, 13))]
    assert (_bits(np.concatenate(pieces)) == _bits(whole)).all()
    # in place through the C ABI: exactly the planes handed over are written, nothing before or behind them
    lib = pkg.load_library()
    buf = np.full((6, W[1], W[0]), 3.25)
    buf[1:5] = v["cn"][4:8]
    assert lib.ekpnp_seed_host(C.byref(p), C.byref(spec), pkg.FIELD_ID["cn"], 4, 4, buf[1:5].ctypes.data_as(C.c_void_p)) == 0
    assert (buf[0] == 3.25).all() and (buf[5] == 3.25).all() and (_bits(buf[1:5]) == _bits(whole[4:8])).all()


def _spec(pkg, **kw):
    d = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-3, noise=0.0, relative=True, seed=1)
    d.update(kw)
    return pkg.seed_spec(**d)


@pytest.mark.parametrize("change, number", [
    (dict(fields=0), "0"),
    (dict(fields=1 << 3), "8"),                      # phi
    (dict(fields=(1 << 1) | (1 << 7)), "130"),        # Ex
    (dict(fields=(1 << 8)), "256"),                   # Ey
    (dict(fields=(1 << 9)), "512"),                   # Ez
    (dict(fields=(1 << 11) | 2), "2050"),             # a bit above 10
    (dict(pattern=4), "4"),
    (dict(pattern=-1), "-1"),
    (dict(modes=(36, 1)), "36"),                      # mx outside 0 .. nx/2 = 35
    (dict(modes=(-1, 1)), "-1"),
    (dict(modes=(1, 34)), "34"),                      # my outside -33 .. 33
    (dict(modes=(1, -34)), "-34"),
    (dict(pattern="hexagons", modes=(1, 17)), "17"),  # |2 my| > ny/2 = 33
    (dict(relative=2), "2"),
    (dict(amplitude=float("nan")), "nan"),
    (dict(amplitude=float("inf")), "inf"),
    (dict(noise=float("-inf")), "-inf"),
])
def test_bad_specs_are_refused_with_the_offending_number(pkg, change, number):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    spec = _spec(pkg, **change)
    assert lib.ekpnp_seed_spec_check(C.byref(p), C.byref(spec)) == INVALID
    msg = lib.ekpnp_last_error(None).decode()
    assert number in msg, msg
    with pytest.raises(pkg.EkpnpError) as e:
        pkg.seed_spec_check(p, spec)
    assert number in str(e.value)
    buf = np.zeros((W[2], W[1], W[0]))
    assert lib.ekpnp_seed_host(C.byref(p), C.byref(spec), 1, 0, W[2], buf.ctypes.data_as(C.c_void_p)) == INVALID
    assert (buf == 0.0).all()


def test_reserved_and_thin_lattices_are_refused_and_good_specs_accepted(pkg):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    spec = _spec(pkg)
    assert lib.ekpnp_seed_spec_check(C.byref(p), C.byref(spec)) == 0
    spec.reserved = 5
    assert lib.ekpnp_seed_spec_check(C.byref(p), C.byref(spec)) == INVALID and "5" in lib.ekpnp_last_error(None).decode()
    spec.reserved = 0
    p.nz = 2
    assert lib.ekpnp_seed_spec_check(C.byref(p), C.byref(spec)) == INVALID
    assert "nz = 2" in lib.ekpnp_last_error(None).decode()
    p = pkg.default_params(*W)
    for good in (_spec(pkg, modes=(35, 33)), _spec(pkg, modes=(0, -33)), _spec(pkg, pattern="hexagons", modes=(1, -16)),
                 _spec(pkg, fields=tuple(SEEDABLE), pattern="none", amplitude=0.0, noise=0.0, relative=False)):
        assert lib.ekpnp_seed_spec_check(C.byref(p), C.byref(good)) == 0, lib.ekpnp_last_error(None)


def test_null_arguments_are_refused_not_dereferenced(pkg):
    lib = pkg.load_library()
    p = pkg.default_params(*W)
    spec = _spec(pkg)
    buf = np.zeros((W[2], W[1], W[0]))
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert lib.ekpnp_seed_spec_check(None, C.byref(spec)) == INVALID
    assert lib.ekpnp_seed_spec_check(C.byref(p), None) == INVALID
    assert lib.ekpnp_seed_host(None, C.byref(spec), 1, 0, W[2], ptr) == INVALID
    assert lib.ekpnp_seed_host(C.byref(p), None, 1, 0, W[2], ptr) == INVALID
    assert lib.ekpnp_seed_host(C.byref(p), C.byref(spec), 1, 0, W[2], None) == INVALID
    assert lib.ekpnp_seed_host(C.byref(p), C.byref(spec), 11, 0, W[2], ptr) == INVALID and "11" in lib.ekpnp_last_error(None).decode()
    assert lib.ekpnp_seed_host(C.byref(p), C.byref(spec), 1, 9, 5, ptr) == INVALID   # planes 9 .. 13 of 13
    assert lib.ekpnp_seed_host(C.byref(p), C.byref(spec), 1, -1, 2, ptr) == INVALID
    assert (buf == 0.0).all()
    assert lib.ekpnp_seed(None, C.byref(spec)) == INVALID
    assert lib.ekpnp_group_seed(None, C.byref(spec)) == INVALID


@pytest.mark.parametrize("flag", ["--seed-pattern", "--modes-every"])
def test_driver_flag_without_a_value_prints_the_usage(pkg, flag):
    assert os.path.exists(EXE), "ekpnp_main not built"
    r = subprocess.run([EXE, flag], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "usage: ekpnp_main" in r.stderr and "--seed-pattern noise|rolls|squares|hexagons" in r.stderr
    for word in ("--seed-modes mx,my", "--seed-amplitude A", "--seed-noise B", "--seed-fields c,cn,...", "--seed-relative 0|1", "--seed N",
                 "--modes-every N", "--modes-field uz", '--modes "m,n;m,n;..."', "modes.dat"):
        assert word in r.stderr, word
    assert "--monitor-every N" in r.stderr and "--batch 1" in r.stderr  # the existing lines are all still there


def test_driver_refuses_unknown_names_by_name(pkg):
    r = subprocess.run([EXE, "--seed-pattern", "stripes"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "stripes" in r.stderr
    r = subprocess.run([EXE, "--seed-pattern", "rolls", "--seed-fields", "c,vorticity"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "vorticity" in r.stderr
    r = subprocess.run([EXE, "--modes-every", "1", "--modes-field", "pressure"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "pressure" in r.stderr
    r = subprocess.run([EXE, "--seed-pattern", "rolls", "--seed-modes", "99,1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "99" in r.stderr
