"""Cost of a coarsened FP32 snapshot (csrc/snapshot.hip) on one grid: the pass itself beside the device's copy rate, and what a
snapshot costs the time loop beside the only route there was without it.

In ONE process, on an in-place context (short creation) of the given grid (default 512x512x513: cz = 2 has to divide nz - 1), every device step under a time
limit of its own (the process ends with a traceback if one runs over):
  (a) per spec 1,1,1 and 2,2,2, all eleven fields: the kernel alone (host clock around begin + synchronize, best of --repeats),
      bytes read (8 B x nodes of the sampled planes x fields) / that time beside ekpnp_copy_bandwidth from the same run, and
      kernel + copy + file (begin ... finish on an idle device)
  (b) wall time of step(n); synchronize - of begin; step(n); finish; synchronize (spec 2,2,2: the file is written while the
      device steps) - and of the route without the pass: get_field of the same fields, the numpy block mean, step(n)
and writes one JSON record (default profiles/snapshot_rate.json) that carries the command line.  Exits non-zero if the extra time
of the begin / finish route over plain stepping is not smaller than the extra time of the get_field route.

    python tools/time_snapshot.py [--grid 512x512x513] [--steps 20] [--repeats 5] [--out FILE] [--limit SECONDS]
"""
import argparse
import faulthandler
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402


class limited:
    """a device step under its own time limit: past it the process prints every thread's stack and exits"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()


def block_mean(a, coarsen):
    """the parent route's host arithmetic: every cz-th plane, cx x cy means, float32 (numpy's own summation order)"""
    cx, cy, cz = coarsen
    v = a[::cz]
    Z, ny, nx = v.shape
    return v.reshape(Z, ny // cy, cy, nx // cx, cx).mean(axis=(2, 4)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", default="512x512x513")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds allowed to one device step of this tool")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_rate.json"))
    a = ap.parse_args()
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    if nx % 2 or ny % 2 or (nz - 1) % 2:
        ap.error("--grid: the spec 2,2,2 wants even nx, ny and nz - 1")
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    rec = {"command": " ".join(["python", "tools/time_snapshot.py"] + sys.argv[1:]), "lattice": [nx, ny, nz], "steps_per_window": a.steps}
    tmp = tempfile.mkdtemp(prefix="ekpnp_snap_")
    path = os.path.join(tmp, "snap.vtk")
    with limited(a.limit):
        s = pkg.Solver(p)
    with s:
        with limited(a.limit):
            s.call("init_fields")  # gpu_initialization: uniform fields
            s.init_equilibrium()
            s.step(2)
            s.synchronize()
        with limited(a.limit):
            rec["copy_probe_GBps"] = round(s.copy_bandwidth(1 << 32), 1)
        # (a) the pass
        rec["pass"] = []
        for co in [(1, 1, 1), (2, 2, 2)]:
            X, Y, Z, payload = pkg.snapshot_extent(p, None, co)
            read_bytes = 8 * len(pkg.FIELDS) * Z * nx * ny
            kernel, whole = [], []
            with limited(a.limit):
                s.snapshot_begin(path, None, co)  # buffers are made here
                s.snapshot_finish()
            for _ in range(a.repeats):
                with limited(a.limit):
                    s.synchronize()
                    t0 = time.perf_counter()
                    s.snapshot_begin(path, None, co)
                    s.synchronize()  # the compute stream only: the kernel is done, the copy goes on
                    t1 = time.perf_counter()
                    s.snapshot_finish()
                    t2 = time.perf_counter()
                kernel.append(t1 - t0)
                whole.append(t2 - t0)
            k = min(kernel)
            rec["pass"].append({
                "coarsen": list(co), "fields": len(pkg.FIELDS), "output": [X, Y, Z], "payload_bytes": payload, "bytes_read": read_bytes,
                "kernel_ms": round(k * 1e3, 3), "kernel_ms_all": [round(v * 1e3, 3) for v in kernel],
                "read_GBps": round(read_bytes / k / 1e9, 1), "ratio_to_copy_probe": round(read_bytes / k / 1e9 / rec["copy_probe_GBps"], 3),
                "kernel_copy_file_ms": round(min(whole) * 1e3, 2),
            })
            print(json.dumps(rec["pass"][-1]), flush=True)
        # (b) cost to the time loop, spec 2,2,2
        co = (2, 2, 2)
        plain, snap = [], []
        for _ in range(a.repeats):
            with limited(a.limit):
                s.synchronize()
                t0 = time.perf_counter()
                s.step(a.steps)
                s.synchronize()
                plain.append(time.perf_counter() - t0)
            with limited(a.limit):
                t0 = time.perf_counter()
                s.snapshot_begin(path, None, co)
                s.step(a.steps)
                s.snapshot_finish()
                s.synchronize()
                snap.append(time.perf_counter() - t0)
        with limited(a.limit):
            s.synchronize()
            t0 = time.perf_counter()
            host = {}
            copy_s = mean_s = 0.0
            for n in pkg.FIELDS:  # one field alive at a time
                t = time.perf_counter()
                f = s.get_field(n)
                copy_s += time.perf_counter() - t
                t = time.perf_counter()
                host[n] = block_mean(f, co)
                mean_s += time.perf_counter() - t
                del f
            s.step(a.steps)
            s.synchronize()
            host_route = time.perf_counter() - t0
        t_plain, t_snap = min(plain), min(snap)
        rec["loop"] = {
            "coarsen": list(co), "step_window_s": round(t_plain, 4), "step_window_s_all": [round(v, 4) for v in plain],
            "begin_step_finish_s": round(t_snap, 4), "begin_step_finish_s_all": [round(v, 4) for v in snap],
            "get_field_route_s": round(host_route, 3), "get_field_copies_s": round(copy_s, 3), "numpy_block_mean_s": round(mean_s, 3),
            "extra_snapshot_s": round(t_snap - t_plain, 4), "extra_get_field_route_s": round(host_route - t_plain, 3),
            "ratio_of_extras": round((host_route - t_plain) / max(t_snap - t_plain, 1e-9), 1),
        }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    try:
        os.remove(path)
        os.rmdir(tmp)
    except OSError:
        pass
    if not (t_snap - t_plain) < (host_route - t_plain):
        sys.exit("the begin / finish route costs the time loop no less than the get_field route")


if __name__ == "__main__":
    main()
