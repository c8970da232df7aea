"""What the tracers' sort by cell (csrc/tracers.hip: k_tracers_sort_*) costs and what it buys, measured on one grid in ONE process.

On an in-place context of the given grid (default 512x512x512, four lattices) after a few seeded steps, for n = 2^24 and 2^20
particles, passive (mu = 0) and with a mobility, nsub = 1, in the manner of tools/time_tracers.py (windows of --calls enqueue-only
calls around one synchronise each, after a warm-up; medians and the spread; the copy probe of the same process beside them):
  (a) an advance of the scattered cloud (RANDOM-seeded: what a stirred cloud becomes);
  (b) the first sort of that cloud: one call and one synchronise at a time, each on a freshly seeded cloud (the scratch exists);
  (c) an advance of the sorted cloud;
  (d) a re-sort after --drift advances of the sorted cloud (nearly sorted input), one call at a time;
  (e) an advance of the GRID-seeded cloud, which lies in memory order by construction, for comparison.
From them: (b + c) / a - the sort earns its place if this is below 1; c / e; the number of advances after which the first sort
is paid back, b / (a - c); and the K from which sorting before every K-th advance costs less than it saves, d / (a - c) (a lower
bound: it takes the advance to stay at (c) between two sorts, as it does while the cloud drifts by less than a cell).
The sorted cloud is read back once per size and its keys are checked to ascend.
Writes one JSON record (default profiles/tracers_sort_cost.json).  Fails without a GPU.

    python tools/time_tracers_sort.py [--grid 512x512x512] [--sizes 24,20] [--calls 20] [--repeats 5] [--drift 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402


def _grid_for(n, nx, ny, nz):
    """gx, gy, gz with gx*gy*gz == n (a power of two), shaped like the lattice as far as powers of two go (tools/time_tracers.py)"""
    g = [1, 1, 1]
    ext = [nx, ny, nz - 2]
    while g[0] * g[1] * g[2] < n:
        k = max(range(3), key=lambda a: ext[a] / g[a])
        g[k] *= 2
    return tuple(g)


def _stats(ms):
    ms = sorted(ms)
    return {"ms": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", default="512x512x512")
    ap.add_argument("--sizes", default="24,20", help="log2 of the particle counts")
    ap.add_argument("--calls", type=int, default=20, help="advance calls per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows (advances) or timed calls (sorts) per case")
    ap.add_argument("--steps", type=int, default=4, help="time steps before the measurement")
    ap.add_argument("--drift", type=int, default=5, help="advances between a sort and the timed re-sort")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_sort_cost.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_tracers_sort.py: no GPU")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    sizes = [1 << int(v) for v in a.sizes.split(",")]
    rec = {"lattice": [nx, ny, nz], "in_place": True, "calls_per_window": a.calls, "windows": a.repeats, "nsub": 1, "drift_advances": a.drift, "sizes": {}}

    with pkg.Solver(p) as s:
        s.call("init_fields")  # as tools/time_tracers.py: uniform fields, c = cn = chargeinf, a seeded pattern, a few steps
        s.call("pbe_concentrations")
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(4, 4), amplitude=1e-2, noise=1e-3, relative=True, seed=1))
        s.fast_Poisson()
        s.init_equilibrium()
        s.step(a.steps)
        s.synchronize()
        rec["copy_GBps"] = round(s.copy_bandwidth(1 << 30), 1)
        umax = max(float(np.abs(s.get_field(k)).max()) for k in ("ux", "uy", "uz"))
        emax = max(float(np.abs(s.get_field(k)).max()) for k in ("Ex", "Ey", "Ez"))
        if not (umax > 0.0 and emax > 0.0):
            sys.exit("time_tracers_sort.py: the fields are at rest")
        h = 0.1 * p.dx / umax   # the fastest particle moves a tenth of a cell per call
        mu = umax / emax
        rec.update(h_s=h, mu=mu, u_max=umax, E_max=emax)

        def advance_windows(m):
            for _ in range(3):
                s.tracers_advance(h, nsub=1, mu=m)
            s.synchronize()
            ms = []
            for _ in range(a.repeats):
                t = time.perf_counter()
                for _ in range(a.calls):
                    s.tracers_advance(h, nsub=1, mu=m)
                s.synchronize()
                ms.append((time.perf_counter() - t) * 1e3 / a.calls)
            return _stats(ms)

        def one_sort():
            s.synchronize()
            t = time.perf_counter()
            s.tracers_sort()
            s.synchronize()
            return (time.perf_counter() - t) * 1e3

        for n in sizes:
            row = rec["sizes"].setdefault(str(n), {})
            scattered = pkg.tracers_spec(n=n, p=p, seed=7)
            ordered = pkg.tracers_spec(grid=_grid_for(n, nx, ny, nz), p=p)
            s.tracers_release()   # (the cloud of the previous size and its scratch)
            before = s.device_bytes()
            s.tracers_seed(scattered)
            one_sort()   # warm-up: the scratch, the ids and the code objects
            row["device_bytes_of_the_sort"] = int(s.device_bytes() - before - (56 * n + ((n + 4095) // 4096 + 1) * 96))
            x, y, z, _, _ = s.tracers_get()
            keys = (np.minimum(z.astype(np.int64), nz - 2) * ny + y.astype(np.int64)) * nx + x.astype(np.int64)
            row["keys_ascend"] = bool((np.diff(keys) >= 0).all())
            del x, y, z, keys
            for kind, m in (("passive", 0.0), ("charged", mu)):
                r = row.setdefault(kind, {})
                s.tracers_seed(scattered)
                r["a_advance_scattered"] = advance_windows(m)
                first = []
                for _ in range(a.repeats):
                    s.tracers_seed(scattered)
                    first.append(one_sort())
                r["b_first_sort"] = _stats(first)
                r["c_advance_sorted"] = advance_windows(m)
                s.tracers_sort()   # (the windows of (c) let the cloud drift further than --drift advances do)
                again = []
                for _ in range(a.repeats):
                    for _ in range(a.drift):
                        s.tracers_advance(h, nsub=1, mu=m)
                    again.append(one_sort())
                r["d_re_sort"] = _stats(again)
                s.tracers_seed(ordered)
                r["e_advance_grid_ordered"] = advance_windows(m)
                A, B, Cc, D, E = (r[k]["ms"] for k in ("a_advance_scattered", "b_first_sort", "c_advance_sorted", "d_re_sort", "e_advance_grid_ordered"))
                r["b_plus_c_over_a"] = round((B + Cc) / A, 3)
                r["a_over_c"] = round(A / Cc, 3)
                r["c_over_e"] = round(Cc / E, 3)
                r["first_sort_paid_back_after_advances"] = round(B / (A - Cc), 2) if A > Cc else None
                r["break_even_K"] = round(D / (A - Cc), 2) if A > Cc else None
                print(f"n {n} {kind}: a {A} ms, b {B} ms, c {Cc} ms, d {D} ms, e {E} ms, (b + c)/a {r['b_plus_c_over_a']}", flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    if not all(v["keys_ascend"] for v in rec["sizes"].values()):
        sys.exit("time_tracers_sort.py: the keys of a sorted cloud do not ascend")


if __name__ == "__main__":
    main()
