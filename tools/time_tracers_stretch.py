"""What carrying the flow-map gradient with the tracers costs (csrc/tracers.hip: k_tracers_advance_tangent, k_stretch_levels, the sort
with a stretch record), measured on one grid in ONE process.

On an in-place context of the given grid (default 512x512x512, four lattices) after a few seeded steps, with 2^--size particles
(default 2^24):
  (i)   `substep`: ekpnp_tracers_advance and ekpnp_tracers_advance_tangent with nsub = 1 on the SAME cloud, in alternating windows of
        --calls enqueue-only calls around one synchronise each, after a warm-up: the median ms per call of either, the spread of the
        windows and their ratio - for a scattered cloud (RANDOM-seeded), one in memory order (GRID-seeded) and the scattered one after
        ekpnp_tracers_sort, passive and with a mobility.  By count a tangent call adds 152 B per particle per CALL (F and e read and
        written once) to the 384 (768) gathered bytes per SUBSTEP; nsub = 1 is so the worst case for the record's traffic.
  (ii)  `levels`: ekpnp_tracers_stretch_levels at 64 and 4096 levels beside the host route - ekpnp_tracers_stretch_get plus numpy -
        median ms of --repeats calls, and whether the two agree (they must: counts are exact).
  (iii) `sort`: ekpnp_tracers_sort of the scattered cloud without and with a stretch record (10 more gathers), median ms of --repeats
        sorts, each of a freshly seeded cloud.
Nothing is gated on a ratio.  The check: the device's tangent advance of 2^--check-n particles equals
ekpnp_tracers_advance_tangent_host on the fields of this very context, bit for bit.
Writes one JSON record (default profiles/tracers_stretch_cost.json).  Fails without a GPU.
  (iv)  With --ab PARENT_TREE (a built checkout of the parent commit) it then runs `bench.py --gpus 1` of this tree and of that one in
        separate processes, in the order parent change change parent parent change, for a context that never begins a record, and
        writes the lines to profiles/tracers_stretch_bench_ab.log; --ab-only runs that alone, from a process that never opens the GPU.

    python tools/time_tracers_stretch.py [--grid 512x512x512] [--size 24] [--calls 20] [--repeats 5] [--out FILE]
                                         [--ab PARENT_TREE [--ab-only]]
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

from time_tracers import _grid_for  # noqa: E402  (tools/ is the script's directory)


def bench_ab(parent, steps, warmup, log):
    """bench.py of both trees, separate processes, parent change change parent parent change"""
    lines, ms = [], {"parent": [], "change": []}
    for k, leg in enumerate(("parent", "change", "change", "parent", "parent", "change")):
        tree = parent if leg == "parent" else ROOT
        r = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--no-cpu-baseline", "--no-batch-ab"],
                           cwd=tree, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(f"time_tracers_stretch.py: bench.py of the {leg} failed ({r.returncode}): {r.stderr[-1500:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        ms[leg].append(json.loads(line)["ms_per_step"])
        lines += [f"== {leg} run {k + 1}", line]
        print(f"{leg} run {k + 1}: {ms[leg][-1]} ms per step", flush=True)
    med = {k: sorted(v)[1] for k, v in ms.items()}
    head = [f"# bench.py --gpus 1 --steps {steps} --warmup {warmup} --no-cpu-baseline --no-batch-ab (cfg3) of this change (\"change\": the flow-map gradient of the tracers,",
            "# csrc/tracers.hip: k_tracers_advance_tangent, k_stretch_*) and of its parent commit (\"parent\", built from a clean export of it with its own Makefile),",
            "# separate processes in ONE call on one MI355X, in the order parent change change parent parent change (tools/time_tracers_stretch.py --ab).",
            "# No tracer entry point is called: a context that never begins a stretch record allocates and launches nothing new.",
            "# ms_per_step  parent: " + " ".join(f"{v:.4f}" for v in ms["parent"]) + f"  (range {min(ms['parent']):.4f} - {max(ms['parent']):.4f}, median {med['parent']:.4f})",
            "#              change: " + " ".join(f"{v:.4f}" for v in ms["change"]) + f"  (range {min(ms['change']):.4f} - {max(ms['change']):.4f}, median {med['change']:.4f})"]
    with open(log, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    return {"parent_ms_per_step": ms["parent"], "change_ms_per_step": ms["change"], "parent_median": med["parent"], "change_median": med["change"]}


def _stats(ms):
    ms = sorted(ms)
    return {"ms_per_call": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", default="512x512x512")
    ap.add_argument("--size", type=int, default=24, help="log2 of the particle count")
    ap.add_argument("--calls", type=int, default=20, help="advance calls per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case and kernel; timed calls per reduction and sort")
    ap.add_argument("--steps", type=int, default=4, help="time steps before the measurement")
    ap.add_argument("--check-n", type=int, default=16, help="log2 of the cloud the device is held against the host on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_stretch_cost.json"))
    ap.add_argument("--ab", default=None, help="a built checkout of the parent commit: run the bench.py A/B against it afterwards")
    ap.add_argument("--ab-log", default=os.path.join(ROOT, "profiles", "tracers_stretch_bench_ab.log"))
    ap.add_argument("--ab-steps", type=int, default=100)
    ap.add_argument("--ab-warmup", type=int, default=20)
    ap.add_argument("--ab-only", action="store_true", help="skip the cost measurement, run the A/B alone")
    a = ap.parse_args()
    if a.ab_only:
        if not a.ab:
            sys.exit("time_tracers_stretch.py: --ab-only needs --ab PARENT_TREE")
        print(json.dumps(bench_ab(os.path.abspath(a.ab), a.ab_steps, a.ab_warmup, a.ab_log)), flush=True)
        return
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_tracers_stretch.py: no GPU")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    n = 1 << a.size
    rec = {"lattice": [nx, ny, nz], "in_place": True, "n": n, "calls_per_window": a.calls, "windows": a.repeats, "nsub": 1,
           "bytes_per_particle_by_count": {"record_per_call": 152, "gathered_per_substep_passive": 384, "gathered_per_substep_charged": 768, "cloud_per_call": 64},
           "substep": {}, "levels": {}, "sort": {}}

    with pkg.Solver(p) as s:
        s.call("init_fields")  # uniform fields (the PB start-up diverges on a channel this tall) ...
        s.call("pbe_concentrations")  # ... and c = cn = chargeinf of the uniform phi
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(4, 4), amplitude=1e-2, noise=1e-3, relative=True, seed=1))
        s.fast_Poisson()
        s.init_equilibrium()
        s.step(a.steps)
        s.synchronize()
        rec["copy_GBps"] = round(s.copy_bandwidth(1 << 30), 1)
        # a substep that moves the fastest particle a tenth of a cell, mu E of the size of u
        umax = max(float(np.abs(s.get_field(k)).max()) for k in ("ux", "uy", "uz"))
        emax = max(float(np.abs(s.get_field(k)).max()) for k in ("Ex", "Ey", "Ez"))
        if not (umax > 0.0 and emax > 0.0):
            sys.exit("time_tracers_stretch.py: the fields are at rest")
        h = 0.1 * p.dx / umax
        mu = umax / emax
        rec.update(h_s=h, mu=mu, u_max=umax, E_max=emax)

        def window(mob, tangent):
            t = time.perf_counter()
            for _ in range(a.calls):
                s.tracers_advance(h, nsub=1, mu=mu if mob else 0.0, stretch=tangent)
            s.synchronize()
            return (time.perf_counter() - t) * 1e3 / a.calls

        def pair(mob):
            """alternating windows, the tangent one first; both kernels see the same drift of the machine and of the cloud"""
            for tangent in (True, False, True, False):
                s.tracers_advance(h, nsub=1, mu=mu if mob else 0.0, stretch=tangent)  # warm-up: code objects, E arrays
            s.synchronize()
            ms = {False: [], True: []}
            for _ in range(a.repeats):
                for tangent in (True, False):
                    ms[tangent].append(window(mob, tangent))
            plain, tangent = _stats(ms[False]), _stats(ms[True])
            return {"plain": plain, "tangent": tangent, "tangent_over_plain": round(tangent["ms_per_call"] / plain["ms_per_call"], 4),
                    "particles_per_s_tangent": round(n / (tangent["ms_per_call"] * 1e-3), 0), "alive_after": float(s.tracers_moments()[0])}

        box = ((0, nx), (0, ny), (1, nz - 2))
        scattered = pkg.tracers_spec(n=n, box=box, p=p, seed=7)
        for order in ("scattered", "ordered", "sorted"):
            spec = pkg.tracers_spec(grid=_grid_for(n, nx, ny, nz), box=box, p=p) if order == "ordered" else scattered
            for mob in (False, True):
                s.tracers_seed(spec)
                if order == "sorted":
                    s.tracers_sort()
                s.tracers_stretch_begin()
                rec["substep"].setdefault(order, {})["charged" if mob else "passive"] = pair(mob)
                print(order, "charged" if mob else "passive", json.dumps(rec["substep"][order]["charged" if mob else "passive"]), flush=True)

        def timed(f, before=None):
            ms, out = [], None
            for k in range(a.repeats + 1):
                if before:
                    before()
                s.synchronize()
                t = time.perf_counter()
                out = f()
                s.synchronize()
                if k:   # the first call is the warm-up
                    ms.append((time.perf_counter() - t) * 1e3)
            return out, round(sorted(ms)[len(ms) // 2], 4)

        # (ii) the histogram of levels on the record the windows left, beside get + numpy
        def host_levels(l_lo, nlevels):
            F, e = s.tracers_stretch_get()
            F = F.reshape(9, -1)
            trc = F[0] * F[0]
            for q in range(1, 9):
                trc = trc + F[q] * F[q]
            ok = (trc > 0.0) & ~np.isnan(trc)
            level = 2 * e[ok].astype(np.int64) + np.frexp(trc[ok])[1] - 1
            return np.bincount(np.clip(level - l_lo + 1, 0, nlevels + 1), minlength=nlevels + 2), int((~ok).sum())

        for nlevels in (64, 4096):
            l_lo = 1 - nlevels // 2
            (dev, none), ms_dev = timed(lambda: s.tracers_stretch_levels(l_lo, nlevels))
            (want, wnone), ms_host = timed(lambda: host_levels(l_lo, nlevels))
            rec["levels"]["levels_%d" % nlevels] = {"l_lo": l_lo, "device_ms": ms_dev, "get_numpy_ms": ms_host, "cells_in_use": int((dev > 0).sum()),
                                                    "equal": bool(np.array_equal(dev, want) and none == wnone)}
        print(json.dumps(rec["levels"]), flush=True)

        # (iii) the sort without and with a record
        def fresh(record):
            def f():
                s.tracers_seed(scattered)
                if record:
                    s.tracers_stretch_begin()
            return f

        _, plain_ms = timed(lambda: s.tracers_sort(), before=fresh(False))
        _, record_ms = timed(lambda: s.tracers_sort(), before=fresh(True))
        rec["sort"] = {"without_record_ms": plain_ms, "with_record_ms": record_ms, "with_over_without": round(record_ms / plain_ms, 4)}
        print(json.dumps(rec["sort"]), flush=True)

        # the device against the definition, on the fields of this very context
        cn = 1 << a.check_n
        spec = pkg.tracers_spec(n=cn, box=box, p=p, seed=11)
        x, y, z = pkg.tracers_seed_host(p, spec)
        u = [s.get_field(k) for k in ("ux", "uy", "uz")]
        E = [s.get_field(k) for k in ("Ex", "Ey", "Ez")]
        want = pkg.tracers_advance_tangent_host(p, u, x, y, z, E=E, mu=mu, h=10.0 * h, nsub=5)
        s.tracers_seed(spec)
        s.tracers_stretch_begin()
        s.tracers_advance(10.0 * h, nsub=5, mu=mu, stretch=True)
        got = (*s.tracers_get(), *s.tracers_stretch_get())
        rec["check_n"] = cn
        rec["check_largest_F_minus_identity"] = float(np.nanmax(np.abs(want[5] - pkg.stretch_identity(x, y, z)[0])))
        rec["device_equals_host_bits"] = bool(all(np.array_equal(np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(w).view(np.uint64)) for g, w in zip(got[:3], want[:3]))
                                              and all(np.array_equal(got[k], want[k]) for k in (3, 4, 6))
                                              and np.array_equal(np.ascontiguousarray(got[5]).view(np.uint64), np.ascontiguousarray(want[5]).view(np.uint64)))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    if not rec["device_equals_host_bits"]:
        sys.exit("time_tracers_stretch.py: the device's tangent advance and ekpnp_tracers_advance_tangent_host differ")
    if not all(v["equal"] for v in rec["levels"].values()):
        sys.exit("time_tracers_stretch.py: the histogram of levels differs from numpy")
    if a.ab:   # after this process's context is gone
        print(json.dumps(bench_ab(os.path.abspath(a.ab), a.ab_steps, a.ab_warmup, a.ab_log)), flush=True)


if __name__ == "__main__":
    main()
