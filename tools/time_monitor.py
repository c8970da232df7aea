"""What an armed monitor (csrc/monitor.hip) adds to a step, measured on one grid in ONE process.

On a context of the given grid (default cfg3, 512x512x512, four lattices; --in-place for the one-buffer form) the legs
    un-armed | plates only (ids 0-3) armed | all eleven quantities armed,   the armed ones at every = 1 and every = 10
are timed alternately, --repeats times round robin: a host clock around ekpnp_step(--steps) that ends in a synchronise, after
--warmup steps of the same leg.  Reported per leg: the ms per step of every repeat, their median and its difference from the
un-armed median.  The volume pass is also timed on its own - --samples monitor_record calls (enqueue only) and one
synchronise, all quantities minus plates only - and its achieved rate is given against the 56 B per node it reads (seven
arrays, once).  Expectation by byte count: 56 / 1 856 of a step when taken at every step, the plates-only set negligible.
Writes one JSON record (default profiles/monitor_cost.json).  Fails without a GPU.

    python tools/time_monitor.py [--grid 512x512x512] [--in-place] [--steps 20] [--warmup 4] [--repeats 3] [--samples 50] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

STEP_BYTES_PER_NODE = 1856  # bench.py's credit for a cfg3 step
VOLUME_BYTES_PER_NODE = 56
PLATES = [0, 1, 2, 3]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", default="512x512x512")
    ap.add_argument("--in-place", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "monitor_cost.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_monitor.py: no GPU")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1 if a.in_place else 0
    nodes = nx * ny * nz
    legs = [("unarmed", None, 0), ("plates_every1", PLATES, 1), ("all_every1", None, 1), ("plates_every10", PLATES, 10), ("all_every10", None, 10)]
    ms = {name: [] for name, _, _ in legs}
    with pkg.Solver(p) as s:
        s.call("init_fields")  # gpu_initialization: uniform fields (the PB start-up diverges on a channel this tall)
        s.fast_Poisson()
        s.init_equilibrium()
        s.step(2)
        s.synchronize()
        capacity = a.steps + a.warmup + a.samples + 8
        for _ in range(a.repeats):
            for name, quantities, every in legs:
                if every:
                    s.monitor_arm(quantities, every=every, capacity=capacity)
                else:
                    s.monitor_disarm()
                s.step(a.warmup)
                s.synchronize()
                t = time.perf_counter()
                s.step(a.steps)
                s.synchronize()
                ms[name].append((time.perf_counter() - t) * 1e3 / a.steps)
        # the passes on their own: enqueue-only records, one synchronise
        alone = {}
        for name, quantities in (("plates", PLATES), ("all", None)):
            s.monitor_arm(quantities, every=1, capacity=capacity)
            for k in range(4):
                s.monitor_record(k, 0.0)
            s.synchronize()
            t = time.perf_counter()
            for k in range(a.samples):
                s.monitor_record(k, 0.0)
            s.synchronize()
            alone[name] = (time.perf_counter() - t) * 1e3 / a.samples
        last = s.monitor_read()[2][-1]
        s.monitor_disarm()
        graph = s.graph_state()
    med = {k: statistics.median(v) for k, v in ms.items()}
    volume_ms = alone["all"] - alone["plates"]
    rec = {
        "lattice": [nx, ny, nz],
        "in_place": bool(a.in_place),
        "steps_timed": a.steps,
        "warmup_steps": a.warmup,
        "repeats": a.repeats,
        "graph_state": graph,
        "ms_per_step": {k: [round(x, 4) for x in v] for k, v in ms.items()},
        "median_ms_per_step": {k: round(v, 4) for k, v in med.items()},
        "added_ms_per_step": {k: round(v - med["unarmed"], 4) for k, v in med.items() if k != "unarmed"},
        "added_share_of_step": {k: round((v - med["unarmed"]) / med["unarmed"], 5) for k, v in med.items() if k != "unarmed"},
        "unarmed_spread_ms": round(max(ms["unarmed"]) - min(ms["unarmed"]), 4),
        "expected_share_by_bytes_every1": round(VOLUME_BYTES_PER_NODE / STEP_BYTES_PER_NODE, 5),
        "row_alone_ms": {k: round(v, 4) for k, v in alone.items()},
        "volume_pass_ms": round(volume_ms, 4),
        "volume_pass_bytes_per_node": VOLUME_BYTES_PER_NODE,
        "volume_pass_GBps": round(VOLUME_BYTES_PER_NODE * nodes / (volume_ms * 1e-3) / 1e9, 1) if volume_ms > 0 else None,
        "last_row": {n: float(v) for n, v in zip(pkg.MONITOR_NAMES, last)},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
