"""Rate of the plane-profile pass (csrc/stats.hip) on one grid, beside the device's copy rate and the host route it replaces.

In ONE process, on an in-place context (short creation) of the given grid (default 512x512x512):
  * ms per ekpnp_stats_accumulate: host clock around a synchronised loop of --samples calls after --warmup calls;
    achieved rate = 88 B (the eleven field arrays, read once) x nodes / time
  * ekpnp_copy_bandwidth (read + write bytes over time of a plain copy): the project's secondary yardstick
  * the only route to the same numbers without the pass: eleven get_field copies plus the numpy sums, timed once
and writes one JSON record (default profiles/plane_sums_rate.json).  Exits non-zero if a sample is not faster than the host route.

    python tools/time_plane_sums.py [--grid 512x512x512] [--samples 50] [--warmup 5] [--out FILE]
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

RECORDED_STEP_MS = 40.6  # one cfg3 step (README.md, round 5)


def host_route(pkg, s):
    """eleven device-to-host copies, then the 24 sums of every plane with numpy on one core"""
    t0 = time.perf_counter()
    f = {n: s.get_field(n).reshape(s.nz_local, -1) for n in pkg.FIELDS}
    t1 = time.perf_counter()
    q = f["c"] - f["cn"]
    pairs = [("ux", "ux"), ("uy", "uy"), ("uz", "uz"), ("c", "c"), ("cn", "cn"), ("T", "T"), ("uz", "T"), ("uz", "c"), ("uz", "cn"),
             (q, "Ex"), (q, "Ez"), ("ux", "uz"), (q, q)]
    arr = lambda k: f[k] if isinstance(k, str) else k  # noqa: E731
    sums = np.stack([f[n].sum(axis=1) for n in pkg.FIELDS] + [(arr(x) * arr(y)).sum(axis=1) for x, y in pairs])  # one product alive at a time
    t2 = time.perf_counter()
    return sums, t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", default="512x512x512")
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plane_sums_rate.json"))
    a = ap.parse_args()
    if a.samples < 50:
        ap.error("--samples: at least 50 (a shorter window measures the clock)")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    nodes = nx * ny * nz
    with pkg.Solver(p) as s:
        s.call("init_fields")  # gpu_initialization: uniform fields, so that the sums are of real values
        s.synchronize()
        for _ in range(a.warmup):
            s.stats_accumulate()
        s.synchronize()
        s.stats_reset()
        t = time.perf_counter()
        for _ in range(a.samples):
            s.stats_accumulate()
        s.synchronize()
        sample_s = (time.perf_counter() - t) / a.samples
        acc, n = s.stats_get()
        copy_gbs = s.copy_bandwidth(1 << 32)
        host_sums, copy_s, sum_s = host_route(pkg, s)
        now = s.plane_sums()
    assert n == a.samples
    scale = np.abs(host_sums).max(axis=1, keepdims=True) + 1e-300
    rate = 88.0 * nodes / sample_s / 1e9
    rec = {
        "lattice": [nx, ny, nz],
        "samples_timed": a.samples,
        "ms_per_sample": round(sample_s * 1e3, 4),
        "bytes_per_node": 88,
        "achieved_GBps": round(rate, 1),
        "copy_probe_GBps": round(copy_gbs, 1),
        "ratio_to_copy_probe": round(rate / copy_gbs, 3),
        "host_route_s": round(copy_s + sum_s, 3),
        "host_route_copy_s": round(copy_s, 3),
        "host_route_numpy_s": round(sum_s, 3),
        "speedup_over_host_route": round((copy_s + sum_s) / sample_s, 1),
        "share_of_recorded_step": round(sample_s * 1e3 / RECORDED_STEP_MS, 4),
        "recorded_step_ms": RECORDED_STEP_MS,
        "max_rel_difference_to_host_sums": float((np.abs(now - host_sums) / scale).max()),
        "running_sum_equals_samples_times_one": bool(np.allclose(acc, a.samples * now, rtol=1e-12, atol=0.0)),
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    if not sample_s < copy_s + sum_s:
        sys.exit("a sample is not faster than the host route")


if __name__ == "__main__":
    main()
