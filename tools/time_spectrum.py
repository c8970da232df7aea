"""What the x-y power spectra (csrc/spectrum.hip) cost, measured on one grid in ONE process.

On an in-place context of the given grid (default 512x512x512, four lattices), after a few warm-up steps:
  - --samples enqueue-only spectrum_record calls around one synchronise, with 1 and with 16 planes armed: ms per record and its
    share of a step;
  - the synchronous all-plane call (shells and peaks of every plane: the planes in batches through one plan), best of three;
  - beside them the host route the feature replaces: get_field and numpy.fft.rfft2 of every plane, binned with the library's
    table.
Writes one JSON record (default profiles/spectrum_cost.json).  Fails without a GPU, if a 1-plane record is not faster than the host
route, or if the device's shells are not the host route's.

    python tools/time_spectrum.py [--grid 512x512x512] [--samples 50] [--step-ms 40.6] [--out FILE]
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
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--step-ms", type=float, default=40.6, help="the step a record is compared with (bench.py's cfg3 headline)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_cost.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_spectrum.py: no GPU")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    shell_of, count = pkg.spectrum_shells(p)
    rec = {"lattice": [nx, ny, nz], "in_place": True, "samples": a.samples, "step_ms": a.step_ms, "nshell": int(len(count)), "field": "c"}
    with pkg.Solver(p) as s:
        s.call("init_fields")  # gpu_initialization: uniform fields (the PB start-up diverges on a channel this tall) ...
        s.call("pbe_concentrations")  # ... and c = cn = chargeinf of the uniform phi: a relative seed needs something to scale
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(2, 3), amplitude=1e-3, noise=1e-4, seed=1))
        s.fast_Poisson()
        s.init_equilibrium()
        s.step(4)
        s.synchronize()
        before = s.device_bytes()
        rec["records"] = {}
        for planes in ([nz // 2], [1 + k * ((nz - 2) // 16) for k in range(16)]):
            s.spectrum_arm("c", planes, capacity=a.samples + 8)
            for k in range(4):
                s.spectrum_record(k, 0.0)
            s.synchronize()
            t = time.perf_counter()
            for k in range(a.samples):
                s.spectrum_record(k, 0.0)
            enqueue_ms = (time.perf_counter() - t) * 1e3 / a.samples
            s.synchronize()
            ms = (time.perf_counter() - t) * 1e3 / a.samples
            rec["records"][str(len(planes))] = {"planes": planes, "ms_per_record": round(ms, 4), "enqueue_ms_per_record": round(enqueue_ms, 4),
                                                "share_of_step": round(ms / a.step_ms, 5)}
        last = s.spectrum_read()
        rec["device_bytes_added"] = int(s.device_bytes() - before)
        s.spectrum_disarm()
        best = None
        for _ in range(3):
            t = time.perf_counter()
            shells, peaks = s.spectrum("c")
            ms = (time.perf_counter() - t) * 1e3
            best = ms if best is None else min(best, ms)
        rec["all_planes_synchronous"] = {"planes": nz, "ms": round(best, 3), "ms_per_plane": round(best / nz, 5), "share_of_step": round(best / a.step_ms, 4)}
        mid = nz // 2
        rec["peak_mid_plane"] = [float(x) for x in peaks[mid]]
        # the host route: the whole field over the bus, one real transform per plane, binned with the library's table
        t = time.perf_counter()
        v = s.get_field("c")
        get_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        w = np.full(nx // 2 + 1, 2.0)
        w[0] = 1.0
        if nx % 2 == 0:
            w[nx // 2] = 1.0
        flat = shell_of.ravel()
        host = np.zeros((nz, len(count)))
        for z in range(nz):
            F = np.fft.rfft2(v[z])
            P = w[None, :] * (F.real * F.real + F.imag * F.imag)
            host[z] = np.bincount(flat, weights=P.ravel(), minlength=len(count))
        fft_ms = (time.perf_counter() - t) * 1e3
        rec["host_route"] = {"get_field_ms": round(get_ms, 2), "rfft2_and_binning_all_planes_ms": round(fft_ms, 2), "ms": round(get_ms + fft_ms, 2)}
    one = rec["records"]["1"]["ms_per_record"]
    rec["host_route_over_one_plane_record"] = round(rec["host_route"]["ms"] / one, 1)
    rec["host_route_over_all_planes_call"] = round(rec["host_route"]["ms"] / rec["all_planes_synchronous"]["ms"], 1)
    scale = np.abs(host).sum(axis=1, keepdims=True)
    rec["largest_shell_difference_to_host_route_over_plane_total"] = float((np.abs(shells - host) / scale).max())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    if not one < rec["host_route"]["ms"]:
        sys.exit(f"time_spectrum.py: a 1-plane record ({one} ms) is not faster than the host route ({rec['host_route']['ms']} ms)")
    if not rec["largest_shell_difference_to_host_route_over_plane_total"] <= 1e-9:
        sys.exit("time_spectrum.py: the device's shells are not the host route's")
    if not np.array_equal(last[2][-1][-1], shells[rec["records"]["16"]["planes"][-1]]):
        sys.exit("time_spectrum.py: the ring's last row is not the synchronous call's")


if __name__ == "__main__":
    main()
