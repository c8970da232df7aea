"""What a histogram record (csrc/hist.hip) costs, measured on one grid in ONE process.

On an in-place context of the given grid (default 512x512x512, four lattices), over the interior planes 1 .. nz-2:
  - --samples enqueue-only hist_record calls around one synchronise, for a 1-D histogram of a field (uz, 128 bins: 8 B per node), of
    q = c - cn (128 bins: 16 B per node) and a 64 x 64 joint histogram of (q, uz) (24 B per node), each on a CONSTANT field (the
    uniform start fields: every lane of a wavefront at one counter) and on a SPREAD field (white noise seeded into c, cn and uz,
    the axes taken from ekpnp_value_range): ms per record, the achieved rate against the bytes the pass reads, its ratio to the
    copy probe and its share of a step;
  - beside them the copy probe (ekpnp_copy_bandwidth, read + write bytes / time), one value_range call, and the host route the
    records replace: get_field and numpy.histogram / numpy.histogram2d.
Writes one JSON record (default profiles/hist_cost.json).  Fails without a GPU, and fails if a record is not faster than its host
route or a row does not add up to the number of nodes.

    python tools/time_hist.py [--grid 512x512x512] [--samples 20] [--step-ms 40.6] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", default="512x512x512")
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--step-ms", type=float, default=40.6, help="the step a record is compared with (bench.py's cfg3 headline)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_cost.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_hist.py: no GPU")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    planes = (1, nz - 2)
    nodes = nx * ny * (nz - 2)
    rec = {"lattice": [nx, ny, nz], "in_place": True, "planes": list(planes), "samples": a.samples, "step_ms": a.step_ms, "records": {}}

    def timed(s, name, kind, spec, nbytes):
        s.hist_arm(spec, planes=planes, capacity=a.samples + 8)
        for k in range(3):
            s.hist_record(k, 0.0)
        s.synchronize()
        t = time.perf_counter()
        for k in range(a.samples):
            s.hist_record(k, 0.0)
        enqueue_ms = (time.perf_counter() - t) * 1e3 / a.samples
        s.synchronize()
        ms = (time.perf_counter() - t) * 1e3 / a.samples
        _, _, counts, nonfinite = s.hist_read(a.samples + 2, 1)
        if int(counts.sum()) + int(nonfinite[0]) != nodes:
            sys.exit(f"time_hist.py: {name} {kind}: the row adds up to {int(counts.sum()) + int(nonfinite[0])}, not to {nodes} nodes")
        gbps = nbytes * nodes / (ms * 1e-3) / 1e9
        rec["records"].setdefault(name, {})[kind] = {
            "ms_per_record": round(ms, 4), "enqueue_ms_per_record": round(enqueue_ms, 4), "bytes_per_node": nbytes, "GBps": round(gbps, 1),
            "ratio_to_copy": round(gbps / rec["copy_GBps"], 4), "share_of_step": round(ms / a.step_ms, 5),
            "cells_used": int((counts > 0).sum()), "largest_cell": int(counts.max())}
        s.hist_disarm()
        return counts[0]

    with pkg.Solver(p) as s:
        s.call("init_fields")  # gpu_initialization: uniform fields (the PB start-up diverges on a channel this tall) ...
        s.call("pbe_concentrations")  # ... and c = cn = chargeinf of the uniform phi
        s.synchronize()
        rec["copy_GBps"] = round(s.copy_bandwidth(1 << 30), 1)
        before = s.device_bytes()
        # the constant case: uz = 0 and q = 0 everywhere
        timed(s, "uz_128", "constant", pkg.hist_spec(("uz", 128, -1.0, 1.0)), 8)
        timed(s, "q_128", "constant", pkg.hist_spec(("q", 128, -1.0, 1.0)), 16)
        timed(s, "q_uz_64x64", "constant", pkg.hist_spec(("q", 64, -1.0, 1.0), ("uz", 64, -1.0, 1.0)), 24)
        # the spread case: white noise in c, cn (relative) and uz (absolute), axes from the measured ranges
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="noise", amplitude=0.0, noise=1e-1, relative=True, seed=1))
        s.seed(pkg.seed_spec(fields=("uz",), pattern="noise", amplitude=0.0, noise=1e-3, relative=False, seed=2))
        s.synchronize()
        t = time.perf_counter()
        rng = {v: s.value_range(v) for v in ("uz", "q")}
        rec["value_range_ms_per_value"] = round((time.perf_counter() - t) * 1e3 / 2, 3)
        ax = {}
        for v, (lo, hi) in rng.items():
            lo, hi = float(lo[1:-1].min()), float(hi[1:-1].max())
            ax[v] = (lo, hi + (hi - lo) * 1e-9)  # (the largest value inside the last bin)
            rec.setdefault("axes", {})[v] = list(ax[v])
        timed(s, "uz_128", "spread", pkg.hist_spec(("uz", 128, *ax["uz"])), 8)
        timed(s, "q_128", "spread", pkg.hist_spec(("q", 128, *ax["q"])), 16)
        joint = timed(s, "q_uz_64x64", "spread", pkg.hist_spec(("q", 64, *ax["q"]), ("uz", 64, *ax["uz"])), 24)
        rec["device_bytes_added"] = int(s.device_bytes() - before)
        # the host route: the fields over the bus, numpy's histograms
        host = {}
        t = time.perf_counter()
        uz = s.get_field("uz")
        get1 = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        h1, _ = np.histogram(uz[1:-1], bins=128, range=ax["uz"])
        host["uz_128"] = {"get_field_ms": round(get1, 2), "histogram_ms": round((time.perf_counter() - t) * 1e3, 2)}
        t = time.perf_counter()
        q = s.get_field("c") - s.get_field("cn")
        get2 = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        h2, _ = np.histogram(q[1:-1], bins=128, range=ax["q"])
        host["q_128"] = {"get_field_ms": round(get2, 2), "histogram_ms": round((time.perf_counter() - t) * 1e3, 2)}
        t = time.perf_counter()
        h3, _, _ = np.histogram2d(q[1:-1].ravel(), uz[1:-1].ravel(), bins=(64, 64), range=(ax["q"], ax["uz"]))
        host["q_uz_64x64"] = {"get_field_ms": round(get1 + get2, 2), "histogram_ms": round((time.perf_counter() - t) * 1e3, 2)}
        for k, v in host.items():
            v["ms"] = round(v["get_field_ms"] + v["histogram_ms"], 2)
            v["over_a_record"] = round(v["ms"] / rec["records"][k]["spread"]["ms_per_record"], 1)
        rec["host_route"] = host
        # numpy's edges are not the library's index function; the totals inside the axes are the same whatever the edges
        rec["inside_counts_equal_numpy"] = bool(int(joint[1:-1, 1:-1].sum()) == int(h3.sum()))
    for k, v in rec["records"].items():
        v["constant_over_spread"] = round(v["constant"]["ms_per_record"] / v["spread"]["ms_per_record"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    for k, v in rec["host_route"].items():
        for kind in ("constant", "spread"):
            ms = rec["records"][k][kind]["ms_per_record"]
            if not ms < v["ms"]:
                sys.exit(f"time_hist.py: a {k} record on a {kind} field ({ms} ms) is not faster than the host route ({v['ms']} ms)")


if __name__ == "__main__":
    main()
