"""What a tracer advance (csrc/tracers.hip) costs, measured on one grid in ONE process.

On an in-place context of the given grid (default 512x512x512, four lattices) after a few seeded steps:
  - ekpnp_tracers_advance with nsub = 1, passive (mu = 0: three arrays gathered) and with a mobility (six arrays), for n = 2^20 and
    2^24 particles, once GRID-seeded over the whole interior (the cloud lies in memory order: neighbouring lanes read neighbouring
    nodes) and once RANDOM-seeded (scattered: what a stirred cloud becomes).  --repeats windows of --calls enqueue-only calls around
    one synchronise each, after a warm-up: the median ms per call and the spread of the windows, particles per second, and the useful
    bytes gathered per second (192 or 384 B per evaluation, two evaluations per substep) beside the copy probe (ekpnp_copy_bandwidth)
    of the same process;
  - the ratio of the scattered to the ordered time: what decides whether a particle sort is worth building;
  - a moments record and a 16 x 16 x 16 cell count of the largest cloud;
  - the host route the advance replaces: three (six) get_field copies plus ekpnp_tracers_advance_host on the same cloud.
Writes one JSON record (default profiles/tracers_cost.json).  Fails without a GPU, and fails if a device call is not faster than its
host route.

    python tools/time_tracers.py [--grid 512x512x512] [--sizes 20,24] [--calls 20] [--repeats 5] [--out FILE]
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
    """gx, gy, gz with gx*gy*gz == n (a power of two), shaped like the lattice as far as powers of two go"""
    g = [1, 1, 1]
    ext = [nx, ny, nz - 2]
    while g[0] * g[1] * g[2] < n:
        k = max(range(3), key=lambda a: ext[a] / g[a])
        g[k] *= 2
    return tuple(g)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", default="512x512x512")
    ap.add_argument("--sizes", default="20,24", help="log2 of the particle counts")
    ap.add_argument("--calls", type=int, default=20, help="advance calls per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case")
    ap.add_argument("--steps", type=int, default=4, help="time steps before the measurement")
    ap.add_argument("--host-n", type=int, default=20, help="log2 of the cloud the host route is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_cost.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_tracers.py: no GPU")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    sizes = [1 << int(v) for v in a.sizes.split(",")]
    rec = {"lattice": [nx, ny, nz], "in_place": True, "calls_per_window": a.calls, "windows": a.repeats, "nsub": 1, "advance": {}}

    with pkg.Solver(p) as s:
        s.call("init_fields")  # uniform fields (the PB start-up diverges on a channel this tall) ...
        s.call("pbe_concentrations")  # ... and c = cn = chargeinf of the uniform phi
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(4, 4), amplitude=1e-2, noise=1e-3, relative=True, seed=1))
        s.fast_Poisson()
        s.init_equilibrium()
        s.step(a.steps)
        s.synchronize()
        rec["copy_GBps"] = round(s.copy_bandwidth(1 << 30), 1)
        before = s.device_bytes()
        # a substep that moves the fastest particle a tenth of a cell (the cloud keeps its order over the timed calls), mu E of the size of u
        umax = max(float(np.abs(s.get_field(k)).max()) for k in ("ux", "uy", "uz"))
        emax = max(float(np.abs(s.get_field(k)).max()) for k in ("Ex", "Ey", "Ez"))
        if not (umax > 0.0 and emax > 0.0):
            sys.exit("time_tracers.py: the fields are at rest")
        h = 0.1 * p.dx / umax
        mu = umax / emax
        rec.update(h_s=h, mu=mu, u_max=umax, E_max=emax)

        def window(mob):
            t = time.perf_counter()
            for _ in range(a.calls):
                s.tracers_advance(h, nsub=1, mu=mu if mob else 0.0)
            enq = (time.perf_counter() - t) * 1e3 / a.calls
            s.synchronize()
            return (time.perf_counter() - t) * 1e3 / a.calls, enq

        for n in sizes:
            row = rec["advance"].setdefault(str(n), {})
            for order in ("ordered", "scattered"):
                spec = pkg.tracers_spec(grid=_grid_for(n, nx, ny, nz), p=p) if order == "ordered" else pkg.tracers_spec(n=n, p=p, seed=7)
                for mob in (False, True):
                    s.tracers_seed(spec)
                    for _ in range(3):
                        s.tracers_advance(h, nsub=1, mu=mu if mob else 0.0)  # warm-up: code objects, and for mu != 0 the E arrays
                    s.synchronize()
                    w = [window(mob) for _ in range(a.repeats)]
                    ms = sorted(v[0] for v in w)
                    med = ms[len(ms) // 2]
                    nbytes = (384 if mob else 192) * 2
                    alive = float(s.tracers_moments()[0])
                    row.setdefault(order, {})["charged" if mob else "passive"] = {
                        "ms_per_call": round(med, 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                        "enqueue_ms_per_call": round(min(v[1] for v in w), 4), "particles_per_s": round(n / (med * 1e-3), 0),
                        "useful_GBps": round(nbytes * n / (med * 1e-3) / 1e9, 1), "ratio_to_copy": round(nbytes * n / (med * 1e-3) / 1e9 / rec["copy_GBps"], 4),
                        "alive_after": alive}
            for kind in ("passive", "charged"):
                row["scattered_over_ordered_" + kind] = round(row["scattered"][kind]["ms_per_call"] / row["ordered"][kind]["ms_per_call"], 3)

        # the largest cloud, scattered: a moments record and a 16^3 cell count
        n = sizes[-1]
        s.tracers_seed(pkg.tracers_spec(n=n, p=p, seed=7))
        s.tracers_arm(capacity=a.calls + 8)
        for k in range(3):
            s.tracers_record(k, 0.0)
        s.synchronize()
        ms = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            for k in range(a.calls):
                s.tracers_record(k, 0.0)
            s.synchronize()
            ms.append((time.perf_counter() - t) * 1e3 / a.calls)
        ms.sort()
        rec["moments_record"] = {"n": n, "ms": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}
        s.tracers_cell_counts((16, 16, 16))
        ms = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            counts, lost = s.tracers_cell_counts((16, 16, 16))
            ms.append((time.perf_counter() - t) * 1e3)
        ms.sort()
        if int(counts.sum()) + lost != n:
            sys.exit(f"time_tracers.py: the cell counts add up to {int(counts.sum()) + lost}, not to {n}")
        rec["cell_counts_16x16x16"] = {"n": n, "ms": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4),
                                       "largest_cell": int(counts.max()), "smallest_cell": int(counts.min())}
        rec["device_bytes_added"] = int(s.device_bytes() - before)

        # the host route on 2^host_n scattered particles: the fields over the bus, the definition on the host
        hn = 1 << a.host_n
        spec = pkg.tracers_spec(n=hn, p=p, seed=7)
        x, y, z = pkg.tracers_seed_host(p, spec)
        host = {}
        t = time.perf_counter()
        u = [s.get_field(k) for k in ("ux", "uy", "uz")]
        get3 = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        want = pkg.tracers_advance_host(p, u, x, y, z, h=h, nsub=1)
        host["passive"] = {"n": hn, "get_field_ms": round(get3, 2), "advance_host_ms": round((time.perf_counter() - t) * 1e3, 2)}
        t = time.perf_counter()
        E = [s.get_field(k) for k in ("Ex", "Ey", "Ez")]
        get6 = get3 + (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        pkg.tracers_advance_host(p, u, x, y, z, E=E, mu=mu, h=h, nsub=1)
        host["charged"] = {"n": hn, "get_field_ms": round(get6, 2), "advance_host_ms": round((time.perf_counter() - t) * 1e3, 2)}
        s.tracers_seed(spec)
        s.tracers_advance(h, nsub=1, mu=0.0)
        got = s.tracers_get()
        rec["device_equals_host_bits"] = bool(all(np.array_equal(np.asarray(g).view(np.uint64), np.asarray(w).view(np.uint64)) for g, w in zip(got[:3], want[:3])))
        for kind, v in host.items():
            v["ms"] = round(v["get_field_ms"] + v["advance_host_ms"], 2)
            dev = rec["advance"].get(str(hn), rec["advance"][str(sizes[0])])["scattered"][kind]["ms_per_call"]
            v["device_ms_per_call"] = dev
            v["over_a_device_call"] = round(v["ms"] / dev, 1)
        rec["host_route"] = host

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    if not rec["device_equals_host_bits"]:
        sys.exit("time_tracers.py: the device advance and ekpnp_tracers_advance_host differ")
    for kind, v in rec["host_route"].items():
        if not v["device_ms_per_call"] < v["ms"]:
            sys.exit(f"time_tracers.py: a {kind} device advance ({v['device_ms_per_call']} ms) is not faster than the host route ({v['ms']} ms)")


if __name__ == "__main__":
    main()
