"""The on-device diagnostics together: one deterministic schedule of `step(k); X; Y` triples over every ordered pair of
observers and every (observer, mutator) / (mutator, observer) pair, run on three twins of one lattice:

  A  every ring armed (monitor, modes, spectrum, hist, section, tracers); does the recording / asynchronous form of an observer
  B  arms nothing; steps one step at a time, takes a monitor_sample after each, and does the synchronous form on the same state
  C  gets the step calls and the mutators only; looked at once, at the very end

A and B carry the same lazy flags whenever both forms of an observer treat them alike, so a form that read stale state would be
wrong in both; B's monitor_sample is therefore also held against current() and umax(), which bring E up to date themselves.

Everything is compared bit for bit.  The one exception are the eight sums of a tracer row once A's cloud has been sorted: the
moments are added in slot order, so a sorted cloud's sums differ from the unsorted twin's in their last bits, and both are held
to the bound tests/test_tracers_sort_gpu.py:221-235 asserts of the moments after a sort (alive, lost, z_min, z_max exactly, each
sum within n * 2**-53 * sum|term| of the exact sum of the twin's cloud).

No GPU at import time: the schedule, the configurations and the ring capacities are plain Python (tests/test_observer_pairs_cpu.py
checks their coverage); run() is what tests/test_observer_pairs_gpu.py calls.  The host steps from a synchronous value to the
expected ring row (energies, ring_spec, hist_row) are the ones the per-recorder ring tests use and are shared with them."""
import math
import os

import numpy as np

OBSERVERS = ("monitor", "modes", "spectrum", "hist", "section", "tracers", "sort", "stats", "snap", "range", "fields", "current", "efield")
MUTATORS = ("lazy", "batch", "set_phi", "set_c", "reinit", "inval", "poisson")
GROUP_REFUSED = ("tracers", "sort", "inval")   # what a slab context refuses (the test_slab_contexts_are_refused tests)
RECORDERS = ("monitor", "modes", "spectrum", "hist", "section", "tracers")
K = (1, 2, 5, 4)   # 1, 2: the eager path; 5, 4: the captured pair (graph_wanted needs nsteps >= 4), 5 leaves the buffer parity flipped

SEED = dict(fields=("c", "cn"), pattern="squares", modes=(1, 1), amplitude=1e-2, noise=1e-4, relative=True, seed=5)
TRACK = [(1, 1), (1, -1), (0, 0), (2, 1)]   # the modes of the ring test of tests/test_modes_gpu.py
SNAP_FIELDS = ("uz", "Ex")
TRACER_GRID = (8, 6, 5)
TRACER_MU = 1e-9

HALVES = (("monitor", "spectrum", "section"), ("modes", "hist", "tracers"))   # which recorders hold every row; the others wrap a ring of 4
SMALL = 4

# id -> lattice, knobs, the monitor's stride, slabs, the half with room for every row, the joint histogram's second axis
CONFIGS = {
    "R": dict(shape=(40, 12, 17), in_place=0, lattices=4, lazy=1, batch=0, every=1, nslabs=1, big=0, second="Ex"),
    "R-inplace-batch": dict(shape=(40, 12, 17), in_place=1, lattices=4, lazy=1, batch=1, every=3, nslabs=1, big=1, second="phi"),
    "R-3lat-eager-E": dict(shape=(40, 12, 17), in_place=0, lattices=3, lazy=0, batch=0, every=2, nslabs=1, big=0, second="phi"),
    "O": dict(shape=(35, 33, 5), in_place=0, lattices=4, lazy=1, batch=0, every=1, nslabs=1, big=1, second="Ex"),
    "B": dict(shape=(130, 70, 4), in_place=0, lattices=4, lazy=1, batch=0, every=2, nslabs=1, big=0, second="phi"),
    "G2": dict(shape=(40, 12, 17), in_place=0, lattices=4, lazy=1, batch=0, every=1, nslabs=2, big=0, second="Ex"),
    # uneven slabs; one chosen plane and a one-plane histogram range: two of the three slabs add rows of zeros
    "G3-inplace": dict(shape=(40, 12, 17), in_place=1, lattices=4, lazy=1, batch=0, every=2, nslabs=3, big=1, second="phi", planes=[6], hist_planes=(6, 6)),
}


# ---- the schedule -------------------------------------------------------------------------------------------------------

def _pairs():
    """every ordered observer pair, every (observer, mutator) and every (mutator, observer) pair, in rounds: a round walks one
    diagonal of its block, so consecutive pairs never share their first operation, and the rounds of the three blocks take turns,
    so the mutators flip the flags all along the schedule and every kind has run twice after a fifth of it"""
    no, nm = len(OBSERVERS), len(MUTATORS)
    out = []
    for d in range(no):
        out += [(OBSERVERS[i], OBSERVERS[(i + d) % no]) for i in range(no)]
        # (each round of the mutators starts one further on: a round of six - the group's - against the four step counts would
        # otherwise bring a mutator back to the same two of them)
        out += [(MUTATORS[(j + d) % nm], OBSERVERS[((j + d) % nm + d) % no]) for j in range(nm)]
        if d < nm:
            out += [(OBSERVERS[i], MUTATORS[(i + d) % nm]) for i in range(no)]
    return out


def schedule(group=False):
    """[(k, X, Y)]: step(k), then X, then Y; k cycles through K along the list.  group: without the kinds a slab context refuses.
    The pairs are taken in the order of _pairs(), except that a pair whose X has not yet followed this position's k, or whose Y
    has not yet been the last operation before a step(5) / step(1) that comes next, goes first (the earliest such pair; never one
    that repeats the X of the triple before).  Deterministic; tests/test_observer_pairs_cpu.py holds the coverage it reaches."""
    left = [(x, y) for x, y in _pairs() if not (group and (x in GROUP_REFUSED or y in GROUP_REFUSED))]
    after_k, before_k, out = set(), set(), []
    while left:
        k, nxt = K[len(out) % len(K)], K[(len(out) + 1) % len(K)]
        ok = [pr for pr in left if not out or pr[0] != out[-1][1]] or left
        gain = [((pr[0], k) not in after_k) + (nxt in (5, 1) and (pr[1], nxt) not in before_k) for pr in ok]
        x, y = ok[gain.index(max(gain))]
        left.remove((x, y))
        after_k.add((x, k))
        before_k.add((y, nxt))
        out.append((k, x, y))
    return out


def recorders(cfg):
    return [r for r in RECORDERS if not (cfg["nslabs"] > 1 and r in GROUP_REFUSED)]


def rows_recorded(cfg, triples):
    """{recorder: rows A records over these triples}: one per operation of its kind, and for the monitor the rows ekpnp_step appends"""
    ops = [op for _, x, y in triples for op in (x, y)]
    n = {r: ops.count(r) for r in recorders(cfg)}
    n["monitor"] += sum(k for k, _, _ in triples) // cfg["every"]
    return n


def capacities(cfg, triples):
    """{recorder: ring rows}: room for every row for one half of the recorders, SMALL for the other"""
    rows = rows_recorded(cfg, triples)
    return {r: max(rows[r], 1) if r in HALVES[cfg["big"]] else SMALL for r in rows}


def settled_index(triples):
    """the first triple after which every kind of these triples has run twice: nothing is allocated from there on (twice, not once:
    the second of the two snapshot staging slots is made by the second snapshot)"""
    kinds = {op for _, x, y in triples for op in (x, y)}
    seen = {}
    for i, (_, x, y) in enumerate(triples):
        for op in (x, y):
            seen[op] = seen.get(op, 0) + 1
        if all(seen.get(kd, 0) >= 2 for kd in kinds):
            return i
    return len(triples)


# ---- the specs --------------------------------------------------------------------------------------------------------

def planes_of(cfg):
    """the chosen planes of the spectrum and section rings: [1, 8, 15] of the ring tests on 17 planes, the same three places elsewhere"""
    nz = cfg["shape"][2]
    return cfg.get("planes") or sorted({1, (nz - 1) // 2, nz - 2})


def hist_planes_of(cfg):
    return cfg.get("hist_planes") or (1, cfg["shape"][2] - 2)


def snap_coarsen(cfg):
    """(2, 2, 1) where 2 divides the axis (a snapshot's cx, cy must divide nx, ny: 35 x 33 is left uncoarsened)"""
    nx, ny, _ = cfg["shape"]
    return (2 if nx % 2 == 0 else 1, 2 if ny % 2 == 0 else 1, 1)


def with_T(cfg):
    return cfg["lattices"] == 4


def monitor_quantities(pkg, cfg):
    return None if with_T(cfg) else [n for n in pkg.MONITOR_NAMES if "T" not in n]


def section_args(cfg):
    """values, across, range, planes: phi makes the record bring a lazy solve's plates up to date"""
    return ["phi", "q", "uz"], "y", (1, cfg["shape"][1] - 2), planes_of(cfg)


def params(pkg, cfg):
    p = pkg.default_params(*cfg["shape"])
    p.pb_iterations = 20
    p.in_place = cfg["in_place"]
    p.n_lattices = cfg["lattices"]
    if p.n_lattices < 4:
        p.Ra = 0.0   # no temperature lattice: no buoyancy (the library refuses the combination otherwise)
    return p


def tracers_spec(pkg, cfg):
    return pkg.tracers_spec(grid=TRACER_GRID, p=params(pkg, cfg))   # a few hundred points on a grid in the interior box


# ---- from a synchronous value to the expected ring row (shared with the per-recorder ring tests) -------------------------------

def energies(ab):
    """[nmodes] from [nmodes][planes][2] in the prescribed order: e = a*a; e = e + b*b; E = E + e, ascending z (Python floats:
    every operation rounded once)"""
    out = []
    for j in range(ab.shape[0]):
        E = 0.0
        for z in range(ab.shape[1]):
            a, b = float(ab[j, z, 0]), float(ab[j, z, 1])
            e = a * a
            e = e + b * b
            E = E + e
        out.append(E)
    return np.array(out)


def group_energies(ab, cuts):
    """a group's row: the slabs' energies added in ascending slab order; cuts: the first plane of every slab and nz"""
    out = energies(ab[:, cuts[0]:cuts[1]])
    for lo, hi in zip(cuts[1:-1], cuts[2:]):
        out = out + energies(ab[:, lo:hi])
    return out


def ring_spec(s, z_lo, z_hi, joint, second="phi"):
    """axes from the start fields' own ranges over the recorded planes, a little narrower so that both outer cells are used"""
    z0 = getattr(s, "z0", 0)
    lo, hi = (v[z_lo - z0:z_hi - z0 + 1] for v in s.value_range("q"))
    qlo, qhi = float(lo.min()), float(hi.max())
    w = qhi - qlo
    assert w > 0.0
    a = ("q", 24, qlo + 0.05 * w, qhi - 0.05 * w)
    if not joint:
        return a, None
    plo, phi = s.value_range(second)
    plo, phi = float(plo.min()), float(phi.max())
    assert phi > plo
    return a, (second, 6, plo + 0.05 * (phi - plo), phi - 0.05 * (phi - plo))


def hist_row(counts, nonfinite, z_lo, z_hi):
    """a ring row from hist_planes: the planes of the range added up"""
    return counts[z_lo:z_hi + 1].sum(axis=0), nonfinite[z_lo:z_hi + 1].sum()


def seeded_start(pkg, s, **knobs):
    for k, v in knobs.items():
        s.tune(k, v)
    s.initialization()
    s.seed(pkg.seed_spec(**SEED))
    s.fast_Poisson()
    s.init_equilibrium()
    return s


# ---- the twins ----------------------------------------------------------------------------------------------------------

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def graph_state(h):
    """of a context, or of every slab of a group"""
    if hasattr(h, "graph_state"):
        return h.graph_state()
    return tuple(int(h._L.ekpnp_graph_state(h.slab_handle(i))) for i in range(h.n))


def _tracer_terms(pkg, p, spec, cloud):
    """the terms of the eight sums of a moments row, from a cloud in id order (tests/test_tracers_sort_gpu.py:224-230)"""
    x, y, z, wx, wy = cloud
    x0, y0, z0 = pkg.tracers_seed_host(p, spec)
    alive = ~np.isnan(x)
    dx = (x[alive] - x0[alive]) + wx[alive].astype(np.float64) * float(p.nx)
    dy = (y[alive] - y0[alive]) + wy[alive].astype(np.float64) * float(p.ny)
    dz = z[alive] - z0[alive]
    za = z[alive]
    return int(alive.sum()), [dx, dy, dz, dx * dx, dy * dy, dz * dz, za, za * za]


def run(pkg, name, tmp, triples=None):
    """the whole schedule of configuration `name` (or the slice / list `triples` of it, to narrow a mismatch by hand) on the three
    twins; files go under the directory tmp.  Returns figures for the caller to print: steps, rows per recorder, the largest fields."""
    cfg = CONFIGS[name]
    group = cfg["nslabs"] > 1
    full = schedule(group)
    if triples is None:
        triples = full
    elif isinstance(triples, slice):
        triples = full[triples]
    p = params(pkg, cfg)
    tmp = str(tmp)
    for d in ("A", "B"):
        os.makedirs(os.path.join(tmp, d), exist_ok=True)

    def make():
        return pkg.Group(p, cfg["nslabs"], devices=[0] * cfg["nslabs"]) if group else pkg.Solver(p)

    with make() as A, make() as B, make() as C:
        twins = (A, B, C)
        for s in twins:
            seeded_start(pkg, s, lazy_efield=cfg["lazy"], batch_moments=cfg["batch"])
        recs = recorders(cfg)
        cap = capacities(cfg, triples)
        quantities = monitor_quantities(pkg, cfg)
        planes = planes_of(cfg)
        z_lo, z_hi = hist_planes_of(cfg)
        hspec = pkg.hist_spec(*ring_spec(B, z_lo, z_hi, True, cfg["second"]))
        sec = section_args(cfg)
        cuts = [A.slab_extent(i)[0] for i in range(cfg["nslabs"])] + [p.nz] if group else None
        A.monitor_arm(quantities, every=cfg["every"], capacity=cap["monitor"])
        A.modes_arm("uz", TRACK, capacity=cap["modes"])
        A.spectrum_arm("uz", planes, capacity=cap["spectrum"])
        A.hist_arm(hspec, planes=(z_lo, z_hi), capacity=cap["hist"])
        A.section_arm(*sec, capacity=cap["section"])
        if not group:
            tspec = tracers_spec(pkg, cfg)
            A.tracers_seed(tspec)
            B.tracers_seed(tspec)
            A.tracers_arm(capacity=cap["tracers"])
        want = {r: [] for r in recs}   # per recorder: (step, time, value ...) of every row A should have recorded, in order
        state = dict(total=0, lazy=cfg["lazy"], batch=cfg["batch"], tracers=0, sorted=False, snaps=0, stats_n=0,
                     stats=np.zeros((len(pkg.PROFILE_NAMES), p.nz)))
        where = ""

        def check(ok, what, *detail):
            assert ok, (f"{name}: {where}: {what}",) + detail

        def compare_fields(hs, labels):
            f = [h.fields() for h in hs]
            for n in pkg.FIELDS:
                for g, lab in zip(f[1:], labels[1:]):
                    check(same(f[0][n], g[n]), f"field {n} of {labels[0]} and {lab} differ", int((bits(f[0][n]) != bits(g[n])).sum()))
            return f[0]

        def apply(op):
            t = state["total"]
            if op == "monitor":
                A.monitor_record(t, A.t)
                row = B.monitor_sample(quantities)
                want["monitor"].append((t, B.t, row))
                # A and B reach this point with the same lazy flags, so a sample that took Ez from a stale array would be wrong in
                # both alike: B's sample is also held against the reference's own verbs, which bring E up to date first
                # (tests/test_monitor_gpu.py:148-149 asserts the same two columns bit for bit)
                cur, um = B.current(), B.umax()
                check(same(row[pkg.MONITOR_ID["current_top"]], cur), "monitor_sample's current_top and current() of B differ", row[0], cur)
                check(same(row[pkg.MONITOR_ID["uz_max"]], um), "monitor_sample's uz_max and umax() of B differ", row[4], um)
            elif op == "modes":
                A.modes_record(t, A.t)
                ab = B.mode_amplitudes("uz", TRACK)
                want["modes"].append((t, B.t, group_energies(ab, cuts) if group else energies(ab)))
            elif op == "spectrum":
                A.spectrum_record(t, A.t)
                want["spectrum"].append((t, B.t, *B.spectrum("uz", planes)))
            elif op == "hist":
                A.hist_record(t, A.t)
                want["hist"].append((t, B.t, *hist_row(*B.hist_planes(hspec), z_lo, z_hi)))
            elif op == "section":
                A.section_record(t, A.t)
                want["section"].append((t, B.t, B.section(*sec)))
            elif op == "tracers":
                mu = TRACER_MU if state["tracers"] % 2 else 0.0   # every other advance is charged: E is then forced
                state["tracers"] += 1
                for s in (A, B):
                    s.tracers_advance(2.0 * p.dt, nsub=2, mu=mu)
                A.tracers_record(t, A.t)
                want["tracers"].append((t, B.t, B.tracers_moments(), B.tracers_get() if state["sorted"] else None))
            elif op == "sort":
                A.tracers_sort()   # changes no trajectory: B does nothing
                state["sorted"] = True
            elif op == "stats":
                A.stats_accumulate()
                state["stats"] = state["stats"] + B.plane_sums()
                state["stats_n"] += 1
            elif op == "snap":
                i = state["snaps"]
                state["snaps"] += 1
                A.snapshot_finish()   # the file of the previous one; this one is written at the next snap or at the end
                A.snapshot_begin(os.path.join(tmp, "A", f"snap_{i}.vtk"), SNAP_FIELDS, snap_coarsen(cfg), time=A.t)
                B.snapshot_begin(os.path.join(tmp, "B", f"snap_{i}.vtk"), SNAP_FIELDS, snap_coarsen(cfg), time=B.t)
                B.snapshot_finish()
            elif op == "range":
                ra, rb = A.value_range("q"), B.value_range("q")
                check(same(ra[0], rb[0]) and same(ra[1], rb[1]), "value_range(q) of A and B differ")
            elif op == "fields":
                compare_fields((A, B), "AB")
            elif op == "current":
                ca, cb, ua, ub = A.current(), B.current(), A.umax(), B.umax()
                check(same(ca, cb), "current() of A and B differ", ca, cb)
                check(same(ua, ub), "umax() of A and B differ", ua, ub)
            elif op == "efield":
                check(same(A.get_field("Ex"), B.get_field("Ex")), "get_field(Ex) of A and B differ")
            elif op in ("lazy", "batch"):
                state[op] ^= 1
                for s in twins:
                    s.tune("lazy_efield" if op == "lazy" else "batch_moments", state[op])
            elif op in ("set_phi", "set_c"):
                n = op[4:]
                v = B.get_field(n) * 1.01   # read from B alone: C is handed the same values without being looked at
                for s in twins:
                    s.set_field(n, v)
            elif op == "reinit":
                for s in twins:
                    s.init_equilibrium()
            elif op == "inval":
                for s in twins:
                    s.invalidate_rhs()
            elif op == "poisson":
                for s in twins:
                    s.fast_Poisson()
            else:
                raise ValueError(op)

        settled, held_bytes = settled_index(triples), None
        for idx, (k, x, y) in enumerate(triples):
            where = f"triple {idx} (k={k}, X={x}, Y={y})"
            A.step(k)
            C.step(k)
            for _ in range(k):
                B.step(1)
                state["total"] += 1
                row = B.monitor_sample(quantities)
                if state["total"] % cfg["every"] == 0:   # the row ekpnp_step itself appends to A's ring
                    want["monitor"].append((state["total"], B.t, row))
            ga, gc = graph_state(A), graph_state(C)
            check(ga == gc, "graph_state of A and C differ after the step", ga, gc)
            where += f" at {x}"
            apply(x)
            where += f" then {y}"
            apply(y)
            now = tuple(s.device_bytes() for s in twins)
            if idx == settled:
                held_bytes = now
            elif idx > settled:
                check(now == held_bytes, "device_bytes of (A, B, C) grew after every kind had run twice", held_bytes, now)

        where = "at the end"
        A.snapshot_finish()
        # 1. every held row of every ring, by label and by bits
        readers = {"monitor": (A.monitor_count, A.monitor_read), "modes": (A.modes_count, A.modes_read), "spectrum": (A.spectrum_count, A.spectrum_read),
                   "hist": (A.hist_count, A.hist_read), "section": (A.section_count, A.section_read)}
        if not group:
            readers["tracers"] = (A.tracers_count, A.tracers_read)
        rows_n = rows_recorded(cfg, triples)
        for r in recs:
            count, read = readers[r]
            n = len(want[r])
            check(n == rows_n[r], f"{r}: the schedule records {rows_n[r]} rows, the runner expected {n}")
            held = min(n, cap[r])
            check(count() == (n, n - held), f"{r}: (recorded, dropped)", count(), (n, n - held))
            if not held:
                continue
            got = read()
            w = want[r][n - held:]
            check(got[0].tolist() == [v[0] for v in w], f"{r}: step labels", got[0].tolist()[:8], [v[0] for v in w][:8])
            check(same(got[1], np.array([v[1] for v in w])), f"{r}: time labels")
            for j, v in enumerate(w):
                tag = f"{r}: row {n - held + j} (step {v[0]})"
                if r == "hist":
                    check(np.array_equal(got[2][j], v[2]) and got[3][j] == v[3], tag)
                elif r == "spectrum":
                    check(same(got[2][j], v[2]), tag + " shells")
                    check(same(got[3][j], v[3]), tag + " peaks")
                elif r == "tracers" and v[3] is not None:   # A's cloud is sorted: the bound of tests/test_tracers_sort_gpu.py:221-235
                    nalive, terms = _tracer_terms(pkg, p, tspec, v[3])
                    for m, who in ((got[2][j], "A"), (v[2], "B")):
                        for q in (0, 1, 10, 11):
                            check(m[q] == v[2][q], tag + f" {pkg.TRACER_MOMENTS[q]} of {who}", m[q], v[2][q])
                        check(m[0] == nalive and m[1] == tspec.n - nalive, tag + f" alive, lost of {who}")
                        for q, t in enumerate(terms):
                            tol = tspec.n * 2.0 ** -53 * np.abs(t).sum()
                            d = abs(m[2 + q] - math.fsum(t))
                            check(d <= tol, tag + f" {pkg.TRACER_MOMENTS[2 + q]} of {who}", d, tol)
                else:
                    check(same(got[2][j], v[2]), tag, got[2][j], v[2])
        # 2. the running profiles
        got, n = A.stats_get()
        check(n == state["stats_n"] and same(got, state["stats"]), "stats_get of A and the host sums of B's plane_sums differ", n, state["stats_n"])
        # 3. the snapshot files
        for i in range(state["snaps"]):
            fa, fb = (os.path.join(tmp, d, f"snap_{i}.vtk") for d in ("A", "B"))
            check(os.path.exists(fa) and os.path.exists(fb), f"snapshot {i} is missing")
            check(open(fa, "rb").read() == open(fb, "rb").read(), f"snapshot {i} of A and B differ")
        # 5. the fields, 6. the checkpoints, 7. the clouds
        f = compare_fields(twins, "ABC")
        for s, d in zip(twins, "ABC"):
            s.save_checkpoint(os.path.join(tmp, f"ck_{d}.bin"))
        ck = [open(os.path.join(tmp, f"ck_{d}.bin"), "rb").read() for d in "ABC"]
        for d in "ABC":
            os.remove(os.path.join(tmp, f"ck_{d}.bin"))   # (tens of megabytes each: not left behind in the test's directory)
        check(ck[0] == ck[1], "save_checkpoint of A and B differ")
        check(ck[0] == ck[2], "save_checkpoint of A and C differ")
        check(A.t == B.t == C.t, "the time of A, B, C", A.t, B.t, C.t)
        if not group:
            ca, cb = A.tracers_get(by_id=True), B.tracers_get(by_id=True)
            for a, b, n in zip(ca, cb, ("x", "y", "z", "wx", "wy")):
                check(same(a, b), f"tracers_get(by_id=True): {n} of A and B differ")
        return dict(triples=len(triples), steps=state["total"], rows={r: len(want[r]) for r in recs}, capacity=cap, snapshots=state["snaps"],
                    checkpoint_bytes=len(ck[0]), nonfinite=int(sum((~np.isfinite(v)).sum() for v in f.values())),
                    largest={n: float(np.nanmax(np.abs(v))) for n, v in f.items()},
                    alive=None if group else int((~np.isnan(ca[0])).sum()))
