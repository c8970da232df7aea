"""Two exact properties of the collide sweep, and everything the two test files that assert them share
(tests/test_equivariance_cpu.py: the CPU oracle; tests/test_equivariance_gpu.py: the HIP path).

1. Shift equivariance.  The lattice is periodic in x and y, and every node runs the same sequence of operations whatever
   its x and y are.  So init_equilibrium followed by k calls of stream_collide_save commutes BIT FOR BIT with
   np.roll(., (sy, sx), axis=(1, 2)) applied to all eleven input fields (Ex, Ey, Ez included: they are held in their arrays,
   no solve runs in between).
2. Locality.  One call moves information by one lattice link.  Two runs whose starts differ at one node may, after s calls,
   differ only inside the Chebyshev ball of radius s around that node - periodic in x, y AND z (gpu_stream wraps z, so a
   plate's change shows on the opposite plate), radius s and not s - 1 (plane z = 0 takes its velocity from node z = 1
   within the same call).

Neither needs a tolerance: every comparison here is np.array_equal or set inclusion, so one ulp at one node fails.  No GPU
or oracle import at module level; the engines are handed in."""
import os
import shutil
import tempfile

import numpy as np

FIELDS = ["rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T"]
LATTICES = ["f", "h", "hn", "temp"]
SHIFT_CALLS = 3
LOCALITY_CALLS = 2
PB_ITERATIONS = 3

# D3Q27 directions in the reference's numbering (LBM.cu:1983-2008): c[d] = (cx, cy, cz)
C27 = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 0), (-1, -1, 0), (1, 0, 1), (-1, 0, -1),
       (0, 1, 1), (0, -1, -1), (1, -1, 0), (-1, 1, 0), (1, 0, -1), (-1, 0, 1), (0, 1, -1), (0, -1, 1), (1, 1, 1), (-1, -1, -1),
       (1, 1, -1), (-1, -1, 1), (1, -1, 1), (-1, 1, -1), (-1, 1, 1), (1, -1, -1)]


def checkpoint_populations(path, p):
    """[lattice][z][y][x][27]: the post-collision populations of a whole-lattice EKPNPCK2 file (layout documented
    in include/ekpnp.h / io.hip: 64-byte header, 11 fields, then per lattice NZ planes of [y][x/64][27 slots][64])."""
    nx, ny, nz, nl = p.nx, p.ny, p.nz, p.n_lattices
    tiles = (nx + 63) // 64
    raw = np.fromfile(path, dtype=np.float64, offset=64)
    nf = 11 * nx * ny * nz
    pops = raw[nf:].reshape(nl, nz, ny, tiles, 27, 64)
    assert raw.size == nf + pops.size
    # since round 5 ("EKPNPCK2") direction d lies in slot 9 (c_z + 1) + 3 (c_y + 1) + (c_x + 1) of its tile
    slot = [9 * (cz + 1) + 3 * (cy + 1) + (cx + 1) for cx, cy, cz in C27]
    assert sorted(slot) == list(range(27))
    pops = pops[:, :, :, :, slot, :]
    return np.moveaxis(pops, 4, 5).reshape(nl, nz, ny, tiles * 64, 27)[:, :, :, :nx, :]


# ---- the cases: data, shared by both test files -------------------------------------------------------------------
# shape (nx, ny, nz); params: members of ekpnp_params set on top of the defaults (both engines); knobs: ekpnp_tune knobs and
# "nslabs" (a Group of that many z slabs on device 0) - they exist in the product only, the oracle ignores them
_FLUID_ONLY = {"n_lattices": 1, "chargeinf": 0.0, "Ra": 0.0, "TH": 0.0}  # what n_lattices = 1 requires (tests/test_parity_gpu.py: cfg1)
CASES = [
    {"id": "16x12x9", "shape": (16, 12, 9)},                                    # k_collide_all, one partial tile
    {"id": "2x2x5", "shape": (2, 2, 5)},                                        # x - 1 and x + 1 are the same node
    {"id": "7x5x4", "shape": (7, 5, 4)},                                        # both plates next to both interior planes
    {"id": "64x3x6", "shape": (64, 3, 6)},                                      # exactly one full tile
    {"id": "130x4x8", "shape": (130, 4, 8)},                                    # three tiles, two live lanes in the last
    {"id": "70x5x9", "shape": (70, 5, 9)},                                      # two tiles, six live lanes
    {"id": "70x5x9-separate-walls", "shape": (70, 5, 9), "knobs": {"merged_walls": 0}},  # k_collide_bulk + k_collide_wall
    {"id": "70x5x19-in-place", "shape": (70, 5, 19), "params": {"in_place": 1}},         # the ordered in-place sweep
    {"id": "70x5x9-nl3", "shape": (70, 5, 9), "params": {"n_lattices": 3, "Ra": 0.0}},
    {"id": "70x5x9-nl1", "shape": (70, 5, 9), "params": _FLUID_ONLY},
    {"id": "70x5x9-moving-wall-body-force", "shape": (70, 5, 9), "params": {"uw": 1e-3, "exf": 1e6}},  # test_moving_wall_and_body_force
    {"id": "16x128x6-ybands", "shape": (16, 128, 6), "knobs": {"merged_walls": 0, "bulk_yband": 64}, "band_rows": 64},
    # z slabs of unequal height: k_collide_faces, k_collide_edge, the halo buffers.  19 planes: 9 + 10 and 6 + 6 + 7;
    # 13 planes in 3 slabs: 4 + 4 + 5, four planes being the least height the library accepts
    {"id": "70x5x19-2slabs", "shape": (70, 5, 19), "knobs": {"nslabs": 2}},
    {"id": "70x5x19-2slabs-in-place", "shape": (70, 5, 19), "params": {"in_place": 1}, "knobs": {"nslabs": 2}},
    {"id": "70x5x19-3slabs", "shape": (70, 5, 19), "knobs": {"nslabs": 3}},
    {"id": "70x5x19-3slabs-in-place", "shape": (70, 5, 19), "params": {"in_place": 1}, "knobs": {"nslabs": 3}},
    {"id": "70x5x13-3slabs", "shape": (70, 5, 13), "knobs": {"nslabs": 3}},
    {"id": "70x5x13-3slabs-in-place", "shape": (70, 5, 13), "params": {"in_place": 1}, "knobs": {"nslabs": 3}},
]
CASE_IDS = [c["id"] for c in CASES]


def case_params(P, case):
    """P: anything with default_params (the oracle module or the package); pb_iterations is 3 in every case"""
    p = P.default_params(*case["shape"])
    p.pb_iterations = PB_ITERATIONS
    for k, v in case.get("params", {}).items():
        setattr(p, k, v)
    return p


def case_shifts(case):
    """(sx, sy): (1, 0), (0, 1), (nx - 1, ny - 1) and, where a row has more than one tile, (63, 1) and (64, ny - 1); shifts that
    are equal modulo the lattice once"""
    nx, ny, _ = case["shape"]
    want = [(1, 0), (0, 1), (nx - 1, ny - 1)] + ([(63, 1), (64, ny - 1)] if nx > 64 else [])
    out = []
    for sx, sy in want:
        s = (sx % nx, sy % ny)
        if s != (0, 0) and s not in out:
            out.append(s)
    return out


def slab_seams(nz, nslabs):
    """first plane of slabs 1 .. nslabs - 1 (the rule of ekpnp_create_slab: slab r begins at r * nz / nslabs)"""
    return [r * nz // nslabs for r in range(1, nslabs)]


def case_locality(case):
    """[((z, y, x), field)]: an interior node at x = 0, y = ny - 1; a plate node at z = 0; a node at z = 1; one at z = nz - 1;
    where nx > 64 the node at x = 64; on a Group one node on each side of every slab seam.  The field rotates through c,
    rho, T (where the lattice exists) and ux."""
    nx, ny, nz = case["shape"]
    nl = case.get("params", {}).get("n_lattices", 4)
    rot = {4: ["c", "rho", "T", "ux"], 3: ["c", "rho", "ux"], 1: ["rho", "ux"]}[nl]
    nodes = [(nz // 2, ny - 1, 0), (0, 1 % ny, nx - 1), (1, 0, nx // 2), (nz - 1, ny // 2, 1 % nx)]
    if nx > 64:
        nodes.append((2, ny - 2, 64))
    for k, z0 in enumerate(slab_seams(nz, case.get("knobs", {}).get("nslabs", 1))):
        nodes += [(z0 - 1, k % ny, 63 % nx), (z0, (k + 2) % ny, (nx - 1 - k) % nx)]
    return [(n, rot[i % len(rot)]) for i, n in enumerate(nodes)]


# ---- the start state ----------------------------------------------------------------------------------------------
def start_state(O, po, seed):
    """All eleven fields, from the oracle: initialization(), O.perturb_fields, seeded noise (relative 1e-3 on c, cn, T, rho;
    absolute 1e-4 on u) so that no two nodes of a plane hold equal values, then one fast_poisson, which leaves phi and the
    Ex, Ey, Ez = efield(phi) the collide will read.  Both engines get these arrays through set_fields."""
    orc = O.Oracle(po)
    try:
        orc.initialization()
        f = O.perturb_fields(po, orc.fields())
        rng = np.random.default_rng(seed)
        for k in ("c", "cn", "T", "rho"):
            f[k] = f[k] * (1.0 + 1e-3 * rng.uniform(-1.0, 1.0, orc.shape))
        for k in ("ux", "uy", "uz"):
            f[k] = f[k] + 1e-4 * rng.uniform(-1.0, 1.0, orc.shape)
        orc.set_fields(f)
        orc.fast_poisson()
        return orc.fields()
    finally:
        orc.close()


# ---- the two engines: create, set_fields, init_equilibrium, stream_collide_save, fields, populations, close ----------
class OracleEngine:
    """the CPU oracle; knobs exist in the product only and are ignored"""

    def __init__(self, O):
        self.O = O

    def create(self, params, knobs):
        e = OracleEngine(self.O)
        e.orc = self.O.Oracle(params)
        e.nlat = 1 if params.n_lattices == 1 else 4  # NLAT of oracle/ekpnp_oracle.c: the lattices its sweeps work on
        return e

    def set_fields(self, d):
        self.orc.set_fields(d)

    def init_equilibrium(self):
        self.orc.init_equilibrium()

    def stream_collide_save(self):
        self.orc.stream_collide_save()

    def fields(self):
        return self.orc.fields()

    def populations(self):
        """lattice -> [79][z][y][x]: X0, then the 26 directions of X1, then those of X2 (Oracle.population(lattice, 0..2))"""
        out = {}
        for lat in LATTICES[:self.nlat]:
            x0, x1, x2 = (self.orc.population(lat, w) for w in (0, 1, 2))
            out[lat] = np.concatenate([x0[None], x1, x2], axis=0)
        return out

    @staticmethod
    def population_label(i):
        return "X0" if i == 0 else f"X1[{i}]" if i <= 26 else f"X2[{i - 26}]"

    def close(self):
        self.orc.close()


class ProductEngine:
    """the library: a Solver, or with knobs["nslabs"] a Group of z slabs on device 0; every other knob goes to tune().  The
    populations are read from a whole-lattice checkpoint."""

    def __init__(self, pkg):
        self.pkg = pkg

    def create(self, params, knobs):
        e = ProductEngine(self.pkg)
        knobs = dict(knobs or {})
        n = knobs.pop("nslabs", 1)
        e.p = params
        e.s = self.pkg.Solver(params) if n == 1 else self.pkg.Group(params, n, devices=[0] * n)
        e.tmp = tempfile.mkdtemp(prefix="ekpnp_equivariance_")
        for k, v in knobs.items():
            e.s.tune(k, v)
        return e

    def set_fields(self, d):
        self.s.set_fields(d)

    def init_equilibrium(self):
        self.s.init_equilibrium()

    def stream_collide_save(self):
        self.s.stream_collide_save()

    def fields(self):
        return self.s.fields()

    def populations(self):
        """lattice -> [27][z][y][x]"""
        path = os.path.join(self.tmp, "state.ck")
        self.s.save_checkpoint(path)
        pops = checkpoint_populations(path, self.p)
        return {LATTICES[l]: np.ascontiguousarray(np.moveaxis(pops[l], 3, 0)) for l in range(self.p.n_lattices)}

    @staticmethod
    def population_label(i):
        return f"direction {i} c = {C27[i]}"

    def close(self):
        self.s.close()
        shutil.rmtree(self.tmp, ignore_errors=True)


# ---- runs -----------------------------------------------------------------------------------------------------------
def run(engine, params, knobs, start, calls, after_create=None):
    """[state after init_equilibrium, after 1 call, ..., after `calls` calls]; a state is name -> array whose last three axes
    are (z, y, x): the eleven fields and one array per lattice (engine.populations)"""
    e = engine.create(params, knobs)
    try:
        if after_create is not None:
            after_create(e)
        e.set_fields(start)
        e.init_equilibrium()
        out = []
        for k in range(calls + 1):
            if k:
                e.stream_collide_save()
            state = dict(e.fields())
            state.update(e.populations())
            out.append(state)
        return out
    finally:
        e.close()


def roll_xy(a, sx, sy):
    return np.roll(a, (sy, sx), axis=(-2, -1))


def _differing_nodes(a, b):
    """bool [z][y][x]: nodes where a and b differ in any leading index (NaN == NaN: the same bits are no difference)"""
    ne = ~((a == b) | ((a != a) & (b != b)))
    return ne.reshape((-1,) + ne.shape[-3:]).any(axis=0)


def check_shift(engine, params, knobs, start, shift, calls, plain=None):
    """init_equilibrium + 0 .. `calls` calls commute with the x-y roll by shift = (sx, sy), bit for bit, in every field and every
    population.  plain: run(engine, params, knobs, start, calls) where the caller has it already."""
    sx, sy = shift
    if plain is None:
        plain = run(engine, params, knobs, start, calls)
    rolled = run(engine, params, knobs, {k: roll_xy(np.asarray(v), sx, sy) for k, v in start.items()}, calls)
    nx, ny = params.nx, params.ny
    for k in range(calls + 1):
        assert sorted(plain[k]) == sorted(rolled[k])
        for name in plain[k]:
            want, got = roll_xy(plain[k][name], sx, sy), rolled[k][name]
            if np.array_equal(want, got, equal_nan=True):
                continue
            ne = ~((want == got) | ((want != want) & (got != got)))
            idx = tuple(int(v) for v in np.argwhere(ne)[0])
            z, y, x = idx[-3:]
            nodes = _differing_nodes(want, got)
            cols = sorted(set(int(v) for v in np.argwhere(nodes)[:, 2]))
            what = f"field {name}" if name in FIELDS else f"lattice {name} {engine.population_label(idx[0])}"
            raise AssertionError(
                f"shift (sx, sy) = ({sx}, {sy}), after {k} calls: {what} of the run from the rolled start is not the rolled {what} of "
                f"the plain run; first differing node (z, y, x) = ({z}, {y}, {x}), tile {x // 64}, lane {x % 64} [node "
                f"({z}, {(y - sy) % ny}, {(x - sx) % nx}), tile {((x - sx) % nx) // 64}, lane {((x - sx) % nx) % 64} of the plain run]: "
                f"{got[idx]!r} vs {want[idx]!r}; {int(nodes.sum())} differing nodes, in the columns x = {cols[:12]}"
                f"{' ...' if len(cols) > 12 else ''} (plain run: x = {sorted(set((c - sx) % nx for c in cols))[:12]})")


def chebyshev_periodic(shape, node):
    """[z][y][x]: the Chebyshev distance of every node from `node`, periodic in all three axes"""
    d = []
    for n, c in zip(shape, node):
        a = np.abs(np.arange(n) - c)
        d.append(np.minimum(a, n - a))
    return np.maximum(np.maximum(d[0][:, None, None], d[1][None, :, None]), d[2][None, None, :])


def check_locality(engine, params, knobs, start, node, field, calls, plain=None):
    """The second run starts with field[node] times 1 + 2**-10 (a velocity component: plus 1e-5).  After s = 1 .. `calls` calls
    the set of nodes where any field or population differs is not empty, contains the node and lies inside the periodic
    Chebyshev ball of radius s."""
    if plain is None:
        plain = run(engine, params, knobs, start, calls)
    changed = {k: np.array(v, dtype=np.float64, copy=True) for k, v in start.items()}
    changed[field][node] = changed[field][node] + 1e-5 if field in ("ux", "uy", "uz") else changed[field][node] * (1.0 + 2.0 ** -10)
    assert changed[field][node] != start[field][node], (field, node, "the start does not change")
    other = run(engine, params, knobs, changed, calls)
    shape = (params.nz, params.ny, params.nx)
    dist = chebyshev_periodic(shape, node)
    for s in range(1, calls + 1):
        differ = np.zeros(shape, dtype=bool)
        for name in plain[s]:
            differ |= _differing_nodes(plain[s][name], other[s][name])
        where = np.argwhere(differ)
        far = tuple(int(v) for v in where[np.argmax(dist[differ])]) if len(where) else None
        msg = (f"{field}{node} changed, after {s} calls: {len(where)} nodes differ, the farthest is {far}"
               f"{'' if far is None else ' at distance ' + str(int(dist[far]))}")
        assert len(where) > 0, msg
        assert differ[node], msg + "; the node itself does not differ"
        assert not (differ & (dist > s)).any(), msg + f"; outside the ball of radius {s}: " + str(
            [tuple(int(v) for v in w) for w in np.argwhere(differ & (dist > s))[:8]])
