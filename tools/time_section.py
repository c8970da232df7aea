"""What a section (csrc/section.hip) costs, measured on one grid in ONE process.

On an in-place context of the given grid (default 512x512x512, four lattices) with white noise in c, cn and uz, across x and
across y, for three value sets - uz (8 B per node), q = c - cn (16 B per node) and all twelve values (88 B per node):
  - the full volume on the device: nz / 16 enqueue-only section_record calls of 16 planes each, which together read every plane
    once, around one synchronise (a ring takes at most 16 planes, and the synchronous call would time the copy of its map too): ms,
    the achieved rate against the bytes read, its ratio to the copy probe and its share of a step;
  - the synchronous call section() of every plane, map copied to the host and all: the figure to hold against the host route;
  - a ring record of 1 plane and of 16 planes (ms per record, enqueue-only calls around one synchronise).
Beside them the copy probe (ekpnp_copy_bandwidth, read + write bytes / time) and the host route a section replaces: get_field and
a numpy sum along the axis.  Writes one JSON record (default profiles/section_cost.json).  Fails without a GPU, and fails if a
pass is not faster than its host route or a map differs from the definition applied to the fetched field.

    python tools/time_section.py [--grid 512x512x512] [--samples 10] [--step-ms 40.6] [--out FILE]
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

SETS = {"uz": (["uz"], 8), "q": (["q"], 16), "all": (None, 88)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", default="512x512x512")
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--step-ms", type=float, default=40.6, help="the step a pass is compared with (bench.py's cfg3 headline)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "section_cost.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_section.py: no GPU")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    rec = {"lattice": [nx, ny, nz], "in_place": True, "samples": a.samples, "step_ms": a.step_ms, "full_volume": {}, "ring": {}}

    def rate(ms, nbytes, planes):
        gbps = nbytes * nx * ny * planes / (ms * 1e-3) / 1e9
        return {"ms": round(ms, 4), "bytes_per_node": nbytes, "TBps": round(gbps / 1e3, 3), "ratio_to_copy": round(gbps / rec["copy_GBps"], 4),
                "share_of_step": round(ms / a.step_ms, 5)}

    def records(s, values, across, groups, repeats):
        """ms per sweep of one enqueue-only record for each group of planes, around one synchronise"""
        total = 0.0
        for planes in groups:
            s.section_arm(values, across, None, planes, capacity=repeats + 4)
            for k in range(2):
                s.section_record(k, 0.0)
            s.synchronize()
            t = time.perf_counter()
            for k in range(repeats):
                s.section_record(k, 0.0)
            s.synchronize()
            total += (time.perf_counter() - t) * 1e3 / repeats
            s.section_disarm()
        return total

    with pkg.Solver(p) as s:
        s.call("init_fields")  # uniform fields (the PB start-up diverges on a channel this tall) ...
        s.call("pbe_concentrations")  # ... and c = cn = chargeinf of the uniform phi
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="noise", amplitude=0.0, noise=1e-1, relative=True, seed=1))
        s.seed(pkg.seed_spec(fields=("uz",), pattern="noise", amplitude=0.0, noise=1e-3, relative=False, seed=2))
        s.synchronize()
        rec["copy_GBps"] = round(s.copy_bandwidth(1 << 30), 1)
        before = s.device_bytes()
        cover = [list(range(z, min(z + 16, nz))) for z in range(0, nz, 16)]
        mid = (nz - 1) // 2
        first16 = list(range(mid - 8, mid + 8)) if nz >= 17 else list(range(nz))
        for across in ("x", "y"):
            full, ring = rec["full_volume"].setdefault("across_" + across, {}), rec["ring"].setdefault("across_" + across, {})
            for name, (values, nbytes) in SETS.items():
                s.section(values, across)  # (the output buffer grows here, not inside the timed calls)
                t = time.perf_counter()
                for _ in range(3):
                    m = s.section(values, across)
                call_ms = (time.perf_counter() - t) * 1e3 / 3
                full[name] = rate(records(s, values, across, cover, 3), nbytes, nz)
                full[name]["synchronous_call_ms"] = round(call_ms, 3)
                if name != "all":
                    ring[name] = {"1_plane": rate(records(s, values, across, [[mid]], a.samples), nbytes, 1),
                                  "16_planes": rate(records(s, values, across, [first16], a.samples), nbytes, len(first16))}
        for name in SETS:
            rec["across_x_over_across_y_" + name] = round(rec["full_volume"]["across_x"][name]["ms"] / rec["full_volume"]["across_y"][name]["ms"], 3)
        rec["device_bytes_added"] = int(s.device_bytes() - before)
        # the host route: the field over the bus, numpy's sum along the axis; and the maps against the definition
        host = {}
        t = time.perf_counter()
        uz = s.get_field("uz")
        get1 = (time.perf_counter() - t) * 1e3
        for across, axis in (("x", 2), ("y", 1)):
            t = time.perf_counter()
            ref = uz.sum(axis=axis)
            host["uz_across_" + across] = {"get_field_ms": round(get1, 2), "numpy_sum_ms": round((time.perf_counter() - t) * 1e3, 2)}
            m = s.section(["uz"], across)[0]
            scale = np.abs(uz).sum(axis=axis)
            if not (np.abs(m - ref) <= 2 * uz.shape[axis] * 2.0 ** -53 * scale).all():
                sys.exit(f"time_section.py: the section of uz across {across} is not the sum of the fetched field")
            z, k = mid, 17 % m.shape[1]
            line = uz[z, k, :] if across == "x" else uz[z, :, k]
            if np.float64(pkg.section_sum(line)).view(np.uint64) != m[z, k].view(np.uint64):
                sys.exit(f"time_section.py: an entry of the section of uz across {across} is not ekpnp_section_sum of its line")
        t = time.perf_counter()
        q = s.get_field("c") - s.get_field("cn")
        get2 = (time.perf_counter() - t) * 1e3
        for across, axis in (("x", 2), ("y", 1)):
            t = time.perf_counter()
            q.sum(axis=axis)
            host["q_across_" + across] = {"get_field_ms": round(get2, 2), "numpy_sum_ms": round((time.perf_counter() - t) * 1e3, 2)}
        for k, v in host.items():
            name, across = k.split("_across_")
            v["ms"] = round(v["get_field_ms"] + v["numpy_sum_ms"], 2)
            v["over_a_synchronous_call"] = round(v["ms"] / rec["full_volume"]["across_" + across][name]["synchronous_call_ms"], 1)
        rec["host_route"] = host
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    for k, v in rec["host_route"].items():
        name, across = k.split("_across_")
        ms = rec["full_volume"]["across_" + across][name]["synchronous_call_ms"]
        if not ms < v["ms"]:
            sys.exit(f"time_section.py: a section of {name} across {across} ({ms} ms, map copied to the host) is not faster than the host route ({v['ms']} ms)")


if __name__ == "__main__":
    main()
