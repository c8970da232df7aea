"""What the absorbing plates of the tracers cost (csrc/tracers.hip: k_tracers_advance_absorbing, k_landings_hist, k_landings_map),
measured on one grid in ONE process.

On an in-place context of the given grid (default 512x512x512, four lattices) after a few seeded steps, with 2^--size particles
(default 2^24):
  (i)   `substep`: ekpnp_tracers_advance_brownian and ekpnp_tracers_advance_absorbing (both plates) with nsub = 1 on the SAME cloud, in
        alternating windows of --calls enqueue-only calls around one synchronise each, after a warm-up: the median ms per call of
        either, the spread of the windows and their ratio - for a scattered cloud (RANDOM-seeded), one in memory order (GRID-seeded)
        and the scattered one after ekpnp_tracers_sort, passive and with a mobility.  The cloud fills the middle half of the channel and
        the kicks are a tenth of a cell: nobody lands (`landed_after` says so), the absorbing kernel does the Brownian one's work plus
        two comparisons per substep.
  (ii)  `half_deposited`: a cloud seeded within a cell of the bottom plate is advanced with kicks of a cell until about half of it has
        landed; then windows of either kernel with kicks of a tenth of a cell, once as the cloud lies and once after ekpnp_tracers_sort.
        Stuck particles share the keys of the plate's plane, so a sort should gather them into wavefronts that leave after the position
        loads; whether that shows is what is measured.  A Brownian substep reflects the stuck particles off the plate, so the windows do
        NOT alternate here: all absorbing windows come first, the landed share is read before and after them, then come the Brownian
        windows on what is then the same cloud for them; the deposit is rebuilt (same seeds: the same cloud, bit for bit) for every case.
  (iii) `reductions`: ekpnp_landings_hist at 64 and 4096 bins and ekpnp_landings_map at 16 x 16 and 256 x 256 cells on the record of (ii),
        each beside the host route - ekpnp_landings_get of the arrays it needs plus numpy - median ms of --repeats calls, and whether
        the two agree (they must: counts are exact).
Nothing is gated on a ratio.  The checks: the device's absorbing advance of 2^16 particles next to the plates equals
ekpnp_tracers_advance_absorbing_host on the same fields, cloud and record, bit for bit; the reductions equal numpy.
Writes one JSON record (default profiles/tracers_absorb_cost.json).  Fails without a GPU.
  (iv)  With --ab PARENT_TREE (a built checkout of the parent commit) it then runs `bench.py --gpus 1` of this tree and of that one in
        separate processes, in the order parent change change parent parent change, for a context that never absorbs, and writes the
        lines to profiles/tracers_absorb_bench_ab.log; --ab-only runs that alone, from a process that never opens the GPU itself.

    python tools/time_tracers_absorb.py [--grid 512x512x512] [--size 24] [--calls 20] [--repeats 5] [--out FILE]
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
            sys.exit(f"time_tracers_absorb.py: bench.py of the {leg} failed ({r.returncode}): {r.stderr[-1500:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        ms[leg].append(json.loads(line)["ms_per_step"])
        lines += [f"== {leg} run {k + 1}", line]
        print(f"{leg} run {k + 1}: {ms[leg][-1]} ms per step", flush=True)
    med = {k: sorted(v)[1] for k, v in ms.items()}
    head = [f"# bench.py --gpus 1 --steps {steps} --warmup {warmup} --no-cpu-baseline --no-batch-ab (cfg3) of this change (\"change\": absorbing plates of the tracers,",
            "# csrc/tracers.hip: k_tracers_advance_absorbing, k_landings_*) and of its parent commit (\"parent\", built from a clean export of it with its own Makefile),",
            "# separate processes in ONE call on one MI355X, in the order parent change change parent parent change (tools/time_tracers_absorb.py --ab).",
            "# No tracer entry point is called: a context that never absorbs allocates and launches nothing new.",
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
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case and kernel; timed calls per reduction")
    ap.add_argument("--steps", type=int, default=4, help="time steps before the measurement")
    ap.add_argument("--check-n", type=int, default=16, help="log2 of the cloud the device is held against the host on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_absorb_cost.json"))
    ap.add_argument("--ab", default=None, help="a built checkout of the parent commit: run the bench.py A/B against it afterwards")
    ap.add_argument("--ab-log", default=os.path.join(ROOT, "profiles", "tracers_absorb_bench_ab.log"))
    ap.add_argument("--ab-steps", type=int, default=100)
    ap.add_argument("--ab-warmup", type=int, default=20)
    ap.add_argument("--ab-only", action="store_true", help="skip the cost measurement, run the A/B alone")
    a = ap.parse_args()
    if a.ab_only:
        if not a.ab:
            sys.exit("time_tracers_absorb.py: --ab-only needs --ab PARENT_TREE")
        print(json.dumps(bench_ab(os.path.abspath(a.ab), a.ab_steps, a.ab_warmup, a.ab_log)), flush=True)
        return
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_tracers_absorb.py: no GPU")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    n = 1 << a.size
    rec = {"lattice": [nx, ny, nz], "in_place": True, "n": n, "calls_per_window": a.calls, "windows": a.repeats, "nsub": 1, "substep": {}, "half_deposited": {}, "reductions": {}}

    with pkg.Solver(p) as s:
        s.call("init_fields")  # uniform fields (the PB start-up diverges on a channel this tall) ...
        s.call("pbe_concentrations")  # ... and c = cn = chargeinf of the uniform phi
        s.seed(pkg.seed_spec(fields=("c", "cn"), pattern="squares", modes=(4, 4), amplitude=1e-2, noise=1e-3, relative=True, seed=1))
        s.fast_Poisson()
        s.init_equilibrium()
        s.step(a.steps)
        s.synchronize()
        rec["copy_GBps"] = round(s.copy_bandwidth(1 << 30), 1)
        # a substep that moves the fastest particle a tenth of a cell, mu E of the size of u, a kick of up to a tenth of a cell
        umax = max(float(np.abs(s.get_field(k)).max()) for k in ("ux", "uy", "uz"))
        emax = max(float(np.abs(s.get_field(k)).max()) for k in ("Ex", "Ey", "Ez"))
        if not (umax > 0.0 and emax > 0.0):
            sys.exit("time_tracers_absorb.py: the fields are at rest")
        h = 0.1 * p.dx / umax
        mu = umax / emax
        D = (0.1 * p.dx) ** 2 / (6.0 * h)
        rec.update(h_s=h, mu=mu, D=D, u_max=umax, E_max=emax)

        def window(mob, absorb):
            t = time.perf_counter()
            for _ in range(a.calls):
                s.tracers_advance(h, nsub=1, mu=mu if mob else 0.0, D=D, seed=5, absorb="both" if absorb else None)
            s.synchronize()
            return (time.perf_counter() - t) * 1e3 / a.calls

        def landed():
            counts, none = s.landings_hist(nbins=1)
            return n - none

        def pair(mob):
            """alternating windows, the absorbing one first; both kernels see the same drift of the machine and of the cloud"""
            for absorb in (True, False, True, False):
                s.tracers_advance(h, nsub=1, mu=mu if mob else 0.0, D=D, seed=5, absorb="both" if absorb else None)  # warm-up: code objects, E arrays, the record
            s.synchronize()
            before = landed()
            ms = {False: [], True: []}
            for _ in range(a.repeats):
                for absorb in (True, False):
                    ms[absorb].append(window(mob, absorb))
            brown, absorbing = _stats(ms[False]), _stats(ms[True])
            return {"brownian": brown, "absorbing": absorbing, "absorbing_over_brownian": round(absorbing["ms_per_call"] / brown["ms_per_call"], 4),
                    "particles_per_s_absorbing": round(n / (absorbing["ms_per_call"] * 1e-3), 0), "landed_before": int(before), "landed_after": int(landed()),
                    "alive_after": float(s.tracers_moments()[0])}

        # (i) plates far away: the middle half of the channel
        box = ((0, nx), (0, ny), (nz // 4, 3 * nz // 4))
        for order in ("scattered", "ordered", "sorted"):
            spec = pkg.tracers_spec(grid=_grid_for(n, nx, ny, nz), box=box, p=p) if order == "ordered" else pkg.tracers_spec(n=n, box=box, p=p, seed=7)
            for mob in (False, True):
                s.tracers_seed(spec)
                if order == "sorted":
                    s.tracers_sort()
                rec["substep"].setdefault(order, {})["charged" if mob else "passive"] = pair(mob)
                print(order, "charged" if mob else "passive", json.dumps(rec["substep"][order]["charged" if mob else "passive"]), flush=True)

        # (ii) about half the cloud on the bottom plate
        big = (1.0 * p.dx) ** 2 / (6.0 * h)
        half = {"rounds": None}

        def deposit():
            s.tracers_seed(pkg.tracers_spec(n=n, box=((0, nx), (0, ny), (0.0, 1.0)), p=p, seed=9))
            rounds = 0
            while rounds < (half["rounds"] or 64):
                s.tracers_advance(h, nsub=1, D=big, seed=6, absorb="bottom")
                rounds += 1
                if half["rounds"] is None and landed() >= n // 2:
                    break
            half["rounds"] = rounds

        def block(mob, absorb):
            for _ in range(2):
                s.tracers_advance(h, nsub=1, mu=mu if mob else 0.0, D=D, seed=5, absorb="bottom" if absorb else None)
            s.synchronize()
            return _stats([window(mob, absorb) for _ in range(a.repeats)])

        for order in ("as_it_lies", "sorted"):
            for mob in (False, True):
                deposit()
                if order == "sorted":
                    s.tracers_sort()
                before = landed()
                absorbing = block(mob, True)
                after = landed()
                brown = block(mob, False)
                rec["half_deposited"].setdefault(order, {})["charged" if mob else "passive"] = {
                    "brownian": brown, "absorbing": absorbing, "absorbing_over_brownian": round(absorbing["ms_per_call"] / brown["ms_per_call"], 4),
                    "landed_before": int(before), "landed_after": int(after)}
                print("half", order, "charged" if mob else "passive", json.dumps(rec["half_deposited"][order]["charged" if mob else "passive"]), flush=True)
        rec["half_deposited"]["rounds_of_a_cell"] = half["rounds"]
        deposit()

        # (iii) the reductions on that record, beside get + numpy
        def timed(f):
            f()
            ms = []
            for _ in range(a.repeats):
                t = time.perf_counter()
                out = f()
                ms.append((time.perf_counter() - t) * 1e3)
            return out, round(sorted(ms)[len(ms) // 2], 4)

        def get(names):
            """ekpnp_landings_get of the named arrays only"""
            import ctypes as C
            types = {"epoch": np.int64, "wall": np.int32, "x": np.float64, "y": np.float64, "wx": np.int32, "wy": np.int32}
            out = {k: np.empty(n, dtype=types[k]) for k in names}
            s._call("landings_get", *[out[k].ctypes.data_as(C.c_void_p) if k in out else None for k in types])
            return out

        top_epoch = s.tracers_epoch()
        for nbins in (64, 4096):
            width = top_epoch // nbins + 1

            def host_hist():
                r = get(("epoch", "wall"))
                e = r["epoch"][r["wall"] != 0]
                return np.bincount(np.minimum(1 + e // width, nbins + 1), minlength=nbins + 2)

            (dev, none), ms_dev = timed(lambda: s.landings_hist(e0=0, width=width, nbins=nbins))
            want, ms_host = timed(host_hist)
            rec["reductions"]["hist_%d" % nbins] = {"device_ms": ms_dev, "get_numpy_ms": ms_host, "equal": bool(np.array_equal(dev, want) and none == n - want.sum())}
        for b in (16, 256):
            def host_map():
                r = get(("epoch", "wall", "x", "y"))
                k = r["wall"] == 1
                cell = (r["y"][k].astype(np.int64) * b // ny) * b + r["x"][k].astype(np.int64) * b // nx
                return np.bincount(cell, minlength=b * b).reshape(b, b)

            (dev, other), ms_dev = timed(lambda: s.landings_map("bottom", (b, b)))
            want, ms_host = timed(host_map)
            rec["reductions"]["map_%dx%d" % (b, b)] = {"device_ms": ms_dev, "get_numpy_ms": ms_host, "equal": bool(np.array_equal(dev, want) and other == n - want.sum())}
        print(json.dumps(rec["reductions"]), flush=True)

        # the device against the definition, on the fields of this very context, next to the plates
        cn = 1 << a.check_n
        spec = pkg.tracers_spec(n=cn, box=((0, nx), (0, ny), (0.0, 1.0)), p=p, seed=11)
        x, y, z = pkg.tracers_seed_host(p, spec)
        u = [s.get_field(k) for k in ("ux", "uy", "uz")]
        want = pkg.tracers_advance_absorbing_host(p, u, x, y, z, D=big, h=h, nsub=3, seed=5, walls=3)
        s.tracers_seed(spec)
        s.tracers_advance(h, nsub=3, D=big, seed=5, absorb="both")
        got = (*s.tracers_get(), *s.landings_get())
        held = want[5] >= 0
        rec["check_n"] = cn
        rec["check_landed"] = int(held.sum())
        rec["device_equals_host_bits"] = bool(all(np.array_equal(np.asarray(g).view(np.uint64), np.asarray(w).view(np.uint64)) for g, w in zip(got[:3], want[:3]))
                                              and all(np.array_equal(got[k], want[k]) for k in (3, 4, 5, 6, 9, 10))
                                              and all(np.array_equal(got[k][held].view(np.uint64), want[k][held].view(np.uint64)) for k in (7, 8)))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    if not rec["device_equals_host_bits"]:
        sys.exit("time_tracers_absorb.py: the device's absorbing advance and ekpnp_tracers_advance_absorbing_host differ")
    if not all(v["equal"] for v in rec["reductions"].values()):
        sys.exit("time_tracers_absorb.py: a reduction of the landing record differs from numpy")
    if a.ab:   # after this process's context is gone
        print(json.dumps(bench_ab(os.path.abspath(a.ab), a.ab_steps, a.ab_warmup, a.ab_log)), flush=True)


if __name__ == "__main__":
    main()
