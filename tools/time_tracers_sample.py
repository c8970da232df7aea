"""What sampling the fields at the tracers and recording tracks (csrc/tracers.hip: k_tracers_sample, k_tracers_track_find,
k_tracers_track_row) cost, measured on one grid in ONE process.

On an in-place context of the given grid (default 512x512x512, four lattices) after a few seeded steps:
  - ekpnp_tracers_sample_device of 1 (T), 3 (ux, uy, uz) and 12 values into a torch tensor, for n = 2^20 and 2^24 particles, on a
    GRID-seeded cloud (memory order), a RANDOM-seeded one (scattered) and that one after ekpnp_tracers_sort (sorted).  --repeats
    windows of --calls enqueue-only calls around one synchronise each, after a warm-up: the median ms per call and the spread of the
    windows, and the useful bytes gathered per second (64 B per array and particle; q reads two arrays) beside the copy probe;
  - beside each order a passive ekpnp_tracers_advance with nsub = 1 on the same cloud - two 24-load evaluations, where a 3-value
    sample is one - and the ratio of the two;
  - the host route a sample replaces, on the smallest cloud: one get_field per array plus ekpnp_tracers_sample_host;
  - ekpnp_tracks_record of 1, 64 and 1024 tags with 0 and 4 values on the largest cloud, never sorted (slot = id: the row kernel
    alone) and sorted (the find pass over the ids, then the row kernel).
Writes one JSON record (default profiles/tracers_sample_cost.json).  With --ab PARENT_TREE (a built checkout of the parent commit)
it then runs `bench.py --gpus 1` of this tree and of that one in separate processes, after its own context is gone, in the order parent
change change parent parent change, for a context that never samples, and writes the lines to profiles/tracers_sample_bench_ab.log.
Fails without a GPU, and fails if the device sample differs from the host's or is not faster than the host route.

    python tools/time_tracers_sample.py [--grid 512x512x512] [--sizes 20,24] [--calls 20] [--repeats 5] [--out FILE] [--ab PARENT_TREE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402
from tools.time_tracers import _grid_for  # noqa: E402

SETS = {1: ("T",), 3: ("ux", "uy", "uz"), 12: ("rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T", "q")}
TRACK_VALUES = ("T", "q", "ux", "uz")


def _arrays(values):
    return sum(2 if v == "q" else 1 for v in values)


def _stat(ms):
    ms = sorted(ms)
    return {"ms_per_call": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def bench_ab(parent, steps, warmup, log):
    """bench.py of both trees, separate processes, parent change change parent parent change"""
    lines, ms = [], {"parent": [], "change": []}
    for k, leg in enumerate(("parent", "change", "change", "parent", "parent", "change")):
        tree = parent if leg == "parent" else ROOT
        r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-batch-ab"],
                           cwd=tree, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"time_tracers_sample.py: bench.py of the {leg} failed ({r.returncode}): {r.stderr[-1500:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        ms[leg].append(json.loads(line)["ms_per_step"])
        lines += [f"== {leg} run {k + 1}", line]
        print(f"{leg} run {k + 1}: {ms[leg][-1]} ms per step", flush=True)
    med = {k: sorted(v)[1] for k, v in ms.items()}
    head = [f"# bench.py --gpus 1 --steps {steps} --warmup {warmup} --no-cpu-baseline --no-batch-ab (cfg3) of this change (\"change\": sampling the fields at the",
            "# tracers and tracks of tagged particles, csrc/tracers.hip) and of its parent commit (\"parent\", built from a clean export of it with its own",
            "# Makefile), separate processes in ONE call on one MI355X, in the order parent change change parent parent change (tools/time_tracers_sample.py",
            "# --ab).  No tracer entry point is called: a context that never samples allocates and launches nothing new.",
            "# ms_per_step  parent: " + " ".join(f"{v:.4f}" for v in ms["parent"]) + f"  (range {min(ms['parent']):.4f} - {max(ms['parent']):.4f}, median {med['parent']:.4f})",
            "#              change: " + " ".join(f"{v:.4f}" for v in ms["change"]) + f"  (range {min(ms['change']):.4f} - {max(ms['change']):.4f}, median {med['change']:.4f})"]
    with open(log, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    return {"parent_ms_per_step": ms["parent"], "change_ms_per_step": ms["change"], "parent_median": med["parent"], "change_median": med["change"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", default="512x512x512")
    ap.add_argument("--sizes", default="20,24", help="log2 of the particle counts")
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case")
    ap.add_argument("--steps", type=int, default=4, help="time steps before the measurement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_sample_cost.json"))
    ap.add_argument("--ab", default=None, help="a built checkout of the parent commit: run the bench.py A/B against it afterwards")
    ap.add_argument("--ab-log", default=os.path.join(ROOT, "profiles", "tracers_sample_bench_ab.log"))
    ap.add_argument("--ab-steps", type=int, default=100)
    ap.add_argument("--ab-warmup", type=int, default=20)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_tracers_sample.py: no GPU")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    sizes = [1 << int(v) for v in a.sizes.split(",")]
    rec = {"lattice": [nx, ny, nz], "in_place": True, "calls_per_window": a.calls, "windows": a.repeats, "sample": {}, "tracks_record": {}}

    with pkg.Solver(p) as s:
        s.call("init_fields")  # uniform fields (the PB start-up diverges on a channel this tall) ...
        s.call("pbe_concentrations")  # ... and c = cn = chargeinf of the uniform phi
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(4, 4), amplitude=1e-2, noise=1e-3, relative=True, seed=1))
        s.fast_Poisson()
        s.init_equilibrium()
        s.step(a.steps)
        s.tracers_seed(n=16, seed=1)
        s.tracers_sample(SETS[12])  # every array as get_field returns it from here on: the timed calls find nothing to bring up to date
        s.synchronize()
        rec["copy_GBps"] = round(s.copy_bandwidth(1 << 30), 1)
        umax = max(float(np.abs(s.get_field(k)).max()) for k in ("ux", "uy", "uz"))
        if not umax > 0.0:
            sys.exit("time_tracers_sample.py: the fields are at rest")
        h = 0.1 * p.dx / umax  # a tenth of a cell: the cloud keeps its order over the timed advances
        out = torch.empty((12, max(sizes)), dtype=torch.float64, device="cuda")

        def windows(call):
            for _ in range(3):
                call()
            s.synchronize()
            ms = []
            for _ in range(a.repeats):
                t = time.perf_counter()
                for _ in range(a.calls):
                    call()
                s.synchronize()
                ms.append((time.perf_counter() - t) * 1e3 / a.calls)
            return _stat(ms)

        for n in sizes:
            row = rec["sample"].setdefault(str(n), {})
            for order in ("ordered", "scattered", "sorted"):
                s.tracers_seed(pkg.tracers_spec(grid=_grid_for(n, nx, ny, nz), p=p) if order == "ordered" else pkg.tracers_spec(n=n, p=p, seed=7))
                if order == "sorted":
                    s.tracers_sort()
                cell = row.setdefault(order, {})
                for nv, values in SETS.items():
                    st = windows(lambda: s.tracers_sample_into(values, out))
                    gb = 64 * _arrays(values) * n / (st["ms_per_call"] * 1e-3) / 1e9
                    st.update(particles_per_s=round(n / (st["ms_per_call"] * 1e-3), 0), useful_GBps=round(gb, 1), ratio_to_copy=round(gb / rec["copy_GBps"], 4))
                    cell[f"{nv}_values"] = st
                adv = windows(lambda: s.tracers_advance(h, nsub=1))
                cell["passive_advance_nsub_1"] = adv
                cell["sample_3_over_advance"] = round(cell["3_values"]["ms_per_call"] / adv["ms_per_call"], 3)

        # the host route on the smallest cloud, scattered: the arrays over the bus, the definition on the host
        hn = sizes[0]
        spec = pkg.tracers_spec(n=hn, p=p, seed=7)
        x, y, z = pkg.tracers_seed_host(p, spec)
        s.tracers_seed(spec)
        host, f = {}, {}
        for nv, values in SETS.items():
            t = time.perf_counter()
            for name in values:
                for arr in (("c", "cn") if name == "q" else (name,)):
                    if arr not in f:
                        f[arr] = s.get_field(arr)
            get_ms = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            want = pkg.tracers_sample_host(p, values, f, x, y, z)
            host_ms = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            got = s.tracers_sample(values)
            dev_ms = (time.perf_counter() - t) * 1e3
            host[f"{nv}_values"] = {"n": hn, "get_field_ms_new_arrays": round(get_ms, 2), "sample_host_ms": round(host_ms, 2), "device_call_with_copy_ms": round(dev_ms, 2),
                                    "device_enqueue_only_ms": rec["sample"][str(hn)]["scattered"][f"{nv}_values"]["ms_per_call"],
                                    "bits_equal": bool(np.array_equal(got.view(np.uint64), want.view(np.uint64)))}
        rec["host_route"] = host
        rec["host_route"]["get_field_ms_all_eleven"] = round(sum(v["get_field_ms_new_arrays"] for v in host.values()), 2)

        # tracks on the largest cloud: never sorted (the row kernel alone), then sorted (the find pass as well)
        n = sizes[-1]
        s.tracers_seed(pkg.tracers_spec(n=n, p=p, seed=7))
        rng = np.random.default_rng(3)
        for state in ("never_sorted", "sorted"):
            if state == "sorted":
                s.tracers_sort()
            for ntags in (1, 64, 1024):
                ids = rng.permutation(n)[:ntags]
                for values in ((), TRACK_VALUES):
                    s.tracks_arm(ids=ids, values=values, capacity=a.calls + 4)
                    rec["tracks_record"].setdefault(state, {})[f"{ntags}_tags_{len(values)}_values"] = windows(lambda: s.tracks_record(0, 0.0))
        s.tracks_disarm()

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def write():
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")

    write()
    print(json.dumps(rec), flush=True)
    for k, v in rec["host_route"].items():
        if isinstance(v, dict):
            if not v["bits_equal"]:
                sys.exit(f"time_tracers_sample.py: the device sample of {k} and ekpnp_tracers_sample_host differ")
            if not v["device_call_with_copy_ms"] < v["sample_host_ms"] + v["get_field_ms_new_arrays"] or not v["device_enqueue_only_ms"] < v["sample_host_ms"]:
                sys.exit(f"time_tracers_sample.py: the device sample of {k} is not faster than the host route")
    if a.ab:
        rec["bench_ab"] = bench_ab(os.path.abspath(a.ab), a.ab_steps, a.ab_warmup, a.ab_log)
        write()
        print(json.dumps(rec["bench_ab"]), flush=True)


if __name__ == "__main__":
    main()
