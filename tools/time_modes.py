"""What a mode record (csrc/modes.hip) and a seed (csrc/seed.hip) cost, measured on one grid in ONE process.

On an in-place context of the given grid (default 512x512x512, four lattices), after a few warm-up steps:
  - --samples enqueue-only modes_record calls around one synchronise, with 1, 4 and 16 modes armed: ms per record, the achieved
    rate against the 8 B per node the pass reads, its ratio to the copy probe and its share of a step;
  - one seed of c, cn (16 B read + 16 B written per interior node), after a warm-up seed with zero amplitudes;
  - beside them the copy probe (ekpnp_copy_bandwidth, read + write bytes / time) and the host route the projection replaces:
    get_field and numpy.fft.rfft2 of every plane.
Writes one JSON record (default profiles/modes_cost.json).  Fails without a GPU, and fails if a 1-mode record is not faster than
the host route.

    python tools/time_modes.py [--grid 512x512x512] [--samples 50] [--step-ms 40.6] [--out FILE]
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

RECORD_BYTES_PER_NODE = 8
SEED_BYTES_PER_NODE_AND_FIELD = 16


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", default="512x512x512")
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--step-ms", type=float, default=40.6, help="the step a record is compared with (bench.py's cfg3 headline)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modes_cost.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_modes.py: no GPU")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    nodes = nx * ny * nz
    rec = {"lattice": [nx, ny, nz], "in_place": True, "samples": a.samples, "step_ms": a.step_ms}
    with pkg.Solver(p) as s:
        s.call("init_fields")  # gpu_initialization: uniform fields (the PB start-up diverges on a channel this tall) ...
        s.call("pbe_concentrations")  # ... and c = cn = chargeinf of the uniform phi: a relative seed needs something to scale
        # the seed: a warm-up call that adds nothing, then the timed one
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(2, 3), amplitude=0.0, noise=0.0))
        s.synchronize()
        t = time.perf_counter()
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(2, 3), amplitude=1e-3, noise=1e-4, seed=1))
        enqueue_ms = (time.perf_counter() - t) * 1e3
        s.synchronize()
        seed_ms = (time.perf_counter() - t) * 1e3
        seed_bytes = 2 * SEED_BYTES_PER_NODE_AND_FIELD * nx * ny * (nz - 2)
        rec["seed_c_cn"] = {"ms": round(seed_ms, 4), "enqueue_ms": round(enqueue_ms, 4), "bytes": seed_bytes,
                            "GBps": round(seed_bytes / (seed_ms * 1e-3) / 1e9, 1)}
        s.fast_Poisson()
        s.init_equilibrium()
        s.step(4)
        s.synchronize()
        copy = s.copy_bandwidth(1 << 30)
        rec["copy_GBps"] = round(copy, 1)
        rec["records"] = {}
        for nm in (1, 4, 16):
            modes = [(2, 3)] + [(k % (nx // 2 + 1), (k * 7) % (ny // 2) - ny // 4) for k in range(1, nm)]
            s.modes_arm("c", modes, capacity=a.samples + 8)
            for k in range(4):
                s.modes_record(k, 0.0)
            s.synchronize()
            t = time.perf_counter()
            for k in range(a.samples):
                s.modes_record(k, 0.0)
            enqueue_ms = (time.perf_counter() - t) * 1e3 / a.samples
            s.synchronize()
            ms = (time.perf_counter() - t) * 1e3 / a.samples
            gbps = RECORD_BYTES_PER_NODE * nodes / (ms * 1e-3) / 1e9
            rec["records"][str(nm)] = {"ms_per_record": round(ms, 4), "enqueue_ms_per_record": round(enqueue_ms, 4), "GBps_at_8B_per_node": round(gbps, 1),
                                       "ratio_to_copy": round(gbps / copy, 4), "share_of_step": round(ms / a.step_ms, 5)}
            if nm == 1:
                rec["E_2_3_last_row"] = float(s.modes_read()[2][-1][0])
        s.modes_disarm()
        # the host route: the whole field over the bus, one real transform per plane
        t = time.perf_counter()
        v = s.get_field("c")
        get_ms = (time.perf_counter() - t) * 1e3
        t = time.perf_counter()
        E = 0.0
        for z in range(nz):
            c = np.fft.rfft2(v[z])[3, 2]
            E += c.real * c.real + c.imag * c.imag
        fft_ms = (time.perf_counter() - t) * 1e3
        rec["host_route"] = {"get_field_ms": round(get_ms, 2), "rfft2_all_planes_ms": round(fft_ms, 2), "ms": round(get_ms + fft_ms, 2), "E_2_3": float(E)}
    one = rec["records"]["1"]["ms_per_record"]
    rec["host_route_over_one_mode_record"] = round(rec["host_route"]["ms"] / one, 1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    if not one < rec["host_route"]["ms"]:
        sys.exit(f"time_modes.py: a 1-mode record ({one} ms) is not faster than the host route ({rec['host_route']['ms']} ms)")
    if not abs(rec["E_2_3_last_row"] - E) <= 1e-9 * abs(E):
        sys.exit(f"time_modes.py: the device's E_2_3 ({rec['E_2_3_last_row']}) is not the host route's ({E})")


if __name__ == "__main__":
    main()
