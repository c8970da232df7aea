"""What the noise of a Brownian tracer advance (csrc/tracers.hip: k_tracers_advance_brownian) costs beside the plain advance,
measured on one grid in ONE process.

On an in-place context of the given grid (default 512x512x512, four lattices) after a few seeded steps, for n = 2^20 and 2^24
particles, for a cloud in memory order (GRID-seeded), a scattered one (RANDOM-seeded) and that scattered cloud after
ekpnp_tracers_sort (ids differ from slots: the kernel reads the id array), passive (mu = 0) and with a mobility:
  - ekpnp_tracers_advance and ekpnp_tracers_advance_brownian with nsub = 1 on the SAME cloud, in alternating windows of --calls
    enqueue-only calls around one synchronise each, after a warm-up: the median ms per call of either and the spread of the windows;
  - their ratio.  A Brownian substep adds one Philox4x32-10 call, three multiply-adds, a fold and a reflection to the 48 (96)
    gathered loads of a plain one; the kicks are a tenth of a cell, so the cloud keeps its order over the timed calls.
Nothing is gated on the ratio.  The one check: the device's Brownian advance of 2^16 scattered particles equals
ekpnp_tracers_advance_brownian_host on the same fields, bit for bit.
Writes one JSON record (default profiles/tracers_brownian_cost.json).  Fails without a GPU.  With --ab PARENT_TREE (a built checkout
of the parent commit) it then runs `bench.py --gpus 1` of this tree and of that one in separate processes, in the order parent change
change parent parent change, for a context that never diffuses, and writes the lines to profiles/tracers_brownian_bench_ab.log;
--ab-only runs that alone, from a process that never opens the GPU itself.

    python tools/time_tracers_brownian.py [--grid 512x512x512] [--sizes 20,24] [--calls 20] [--repeats 5] [--out FILE]
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
            sys.exit(f"time_tracers_brownian.py: bench.py of the {leg} failed ({r.returncode}): {r.stderr[-1500:]}")
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        ms[leg].append(json.loads(line)["ms_per_step"])
        lines += [f"== {leg} run {k + 1}", line]
        print(f"{leg} run {k + 1}: {ms[leg][-1]} ms per step", flush=True)
    med = {k: sorted(v)[1] for k, v in ms.items()}
    head = [f"# bench.py --gpus 1 --steps {steps} --warmup {warmup} --no-cpu-baseline --no-batch-ab (cfg3) of this change (\"change\": Brownian tracers,",
            "# csrc/tracers.hip: k_tracers_advance_brownian) and of its parent commit (\"parent\", built from a clean export of it with its own Makefile),",
            "# separate processes in ONE call on one MI355X, in the order parent change change parent parent change (tools/time_tracers_brownian.py --ab).",
            "# No tracer entry point is called: a context that never diffuses allocates and launches nothing new.",
            "# ms_per_step  parent: " + " ".join(f"{v:.4f}" for v in ms["parent"]) + f"  (range {min(ms['parent']):.4f} - {max(ms['parent']):.4f}, median {med['parent']:.4f})",
            "#              change: " + " ".join(f"{v:.4f}" for v in ms["change"]) + f"  (range {min(ms['change']):.4f} - {max(ms['change']):.4f}, median {med['change']:.4f})"]
    with open(log, "w") as f:
        f.write("\n".join(head + lines) + "\n")
    return {"parent_ms_per_step": ms["parent"], "change_ms_per_step": ms["change"], "parent_median": med["parent"], "change_median": med["change"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--grid", default="512x512x512")
    ap.add_argument("--sizes", default="20,24", help="log2 of the particle counts")
    ap.add_argument("--calls", type=int, default=20, help="advance calls per timed window")
    ap.add_argument("--repeats", type=int, default=5, help="timed windows per case and kernel")
    ap.add_argument("--steps", type=int, default=4, help="time steps before the measurement")
    ap.add_argument("--check-n", type=int, default=16, help="log2 of the cloud the device is held against the host on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tracers_brownian_cost.json"))
    ap.add_argument("--ab", default=None, help="a built checkout of the parent commit: run the bench.py A/B against it afterwards")
    ap.add_argument("--ab-log", default=os.path.join(ROOT, "profiles", "tracers_brownian_bench_ab.log"))
    ap.add_argument("--ab-steps", type=int, default=100)
    ap.add_argument("--ab-warmup", type=int, default=20)
    ap.add_argument("--ab-only", action="store_true", help="skip the cost measurement, run the A/B alone")
    a = ap.parse_args()
    if a.ab_only:
        if not a.ab:
            sys.exit("time_tracers_brownian.py: --ab-only needs --ab PARENT_TREE")
        print(json.dumps(bench_ab(os.path.abspath(a.ab), a.ab_steps, a.ab_warmup, a.ab_log)), flush=True)
        return
    import torch

    if not torch.cuda.is_available():
        sys.exit("time_tracers_brownian.py: no GPU")
    pkg = G.load_package()
    nx, ny, nz = (int(v) for v in a.grid.split("x"))
    p = pkg.default_params(nx, ny, nz)
    p.in_place = 1
    sizes = [1 << int(v) for v in a.sizes.split(",")]
    rec = {"lattice": [nx, ny, nz], "in_place": True, "calls_per_window": a.calls, "windows": a.repeats, "nsub": 1, "advance": {}}

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
            sys.exit("time_tracers_brownian.py: the fields are at rest")
        h = 0.1 * p.dx / umax
        mu = umax / emax
        D = (0.1 * p.dx) ** 2 / (6.0 * h)
        rec.update(h_s=h, mu=mu, D=D, u_max=umax, E_max=emax)

        def window(mob, noise):
            t = time.perf_counter()
            for _ in range(a.calls):
                s.tracers_advance(h, nsub=1, mu=mu if mob else 0.0, D=D if noise else None, seed=5)
            s.synchronize()
            return (time.perf_counter() - t) * 1e3 / a.calls

        def stats(ms):
            ms = sorted(ms)
            return {"ms_per_call": round(ms[len(ms) // 2], 4), "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}

        for n in sizes:
            row = rec["advance"].setdefault(str(n), {})
            for order in ("ordered", "scattered", "sorted"):
                spec = pkg.tracers_spec(grid=_grid_for(n, nx, ny, nz), p=p) if order == "ordered" else pkg.tracers_spec(n=n, p=p, seed=7)
                for mob in (False, True):
                    s.tracers_seed(spec)
                    if order == "sorted":
                        s.tracers_sort()
                    for noise in (False, True, False, True):
                        s.tracers_advance(h, nsub=1, mu=mu if mob else 0.0, D=D if noise else None, seed=5)  # warm-up: code objects, E arrays
                    s.synchronize()
                    ms = {False: [], True: []}
                    for _ in range(a.repeats):   # alternating: both kernels see the same drift of the machine and of the cloud
                        for noise in (False, True):
                            ms[noise].append(window(mob, noise))
                    plain, brown = stats(ms[False]), stats(ms[True])
                    row.setdefault(order, {})["charged" if mob else "passive"] = {
                        "plain": plain, "brownian": brown, "brownian_over_plain": round(brown["ms_per_call"] / plain["ms_per_call"], 4),
                        "particles_per_s_brownian": round(n / (brown["ms_per_call"] * 1e-3), 0), "alive_after": float(s.tracers_moments()[0]),
                        "epoch_after": s.tracers_epoch()}

        # the device against the definition, on the fields of this very context
        cn = 1 << a.check_n
        spec = pkg.tracers_spec(n=cn, p=p, seed=11)
        x, y, z = pkg.tracers_seed_host(p, spec)
        u = [s.get_field(k) for k in ("ux", "uy", "uz")]
        want = pkg.tracers_advance_brownian_host(p, u, x, y, z, D=D, h=h, nsub=3, seed=5)
        s.tracers_seed(spec)
        s.tracers_advance(h, nsub=3, D=D, seed=5)
        got = s.tracers_get()
        rec["check_n"] = cn
        rec["device_equals_host_bits"] = bool(all(np.array_equal(np.asarray(g).view(np.uint64), np.asarray(w).view(np.uint64)) for g, w in zip(got[:3], want[:3]))
                                              and np.array_equal(got[3], want[3]) and np.array_equal(got[4], want[4]))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)
    if not rec["device_equals_host_bits"]:
        sys.exit("time_tracers_brownian.py: the device's Brownian advance and ekpnp_tracers_advance_brownian_host differ")
    if a.ab:   # after this process's context is gone
        print(json.dumps(bench_ab(os.path.abspath(a.ab), a.ab_steps, a.ab_warmup, a.ab_log)), flush=True)


if __name__ == "__main__":
    main()
