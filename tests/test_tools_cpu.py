"""The trace tools under tools/ run on a committed excerpt of a REAL rocprofv3 kernel trace, so that a kernel that is renamed
or leaves the step shows up as a failing test and not - as in round 4 - as empty evidence (VERDICT r04 item 1:
profiles/r04_*_slab_overlap.json were `{"steps": []}` because the tools looked for k_halo_unpack).

tests/golden/trace_excerpt_slab.csv: the last three steps of profiles/r05_cfg5_rank_shape_slab_* (1024x1024x128 through the
multi-rank code path on one rank, HEAD of round 5), written by tools/trace_steps.py --excerpt: data, no source text."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE = os.path.join(ROOT, "tests", "golden", "trace_excerpt_slab.csv")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_steps_are_cut_at_the_boundary_plane_launch():
    import trace_steps as ts

    rows = ts.load_rows(TRACE)
    starts = ts.step_starts(rows)
    assert len(starts) == 4 and all("k_collide_faces" in rows[i]["n"] for i in starts)
    steps = ts.split_steps(rows)
    assert len(steps) == 4 and len(steps[-1]) == 1  # three full steps + the launch that opens the fourth
    for st in steps[:3]:
        sweep = ts.sweep_of(st)
        assert len(sweep) == 2 and sweep[0]["gx"] < sweep[1]["gx"]  # lead-in launch, then the rest of the interior planes
        names = [ts.short_name(r["n"]) for r in st]
        # the step as the library runs it today: no pack / unpack kernels, one exchange kernel beside the sweep
        assert not any("k_halo_pack" in n or "k_halo_unpack" in n for n in names)
        assert sum(ts.is_rccl(r["n"]) for r in st) >= 2


def test_overlap_trace_finds_the_exchange_inside_the_sweep():
    import overlap_trace as ot
    import trace_steps as ts

    res = ot.analyse(ts.load_rows(TRACE))
    assert res["steps_seen"] == 3
    s = res["summary"]
    assert s["steps_with_an_exchange_beside_the_sweep"] == 3 and s["hidden"] is True
    # 1024 x 1024 planes: 302 MB per face and direction leave the ring in ~1.8 ms of a ~38.7 ms sweep
    assert 1.0 < s["exchange_ends_ms_after_sweep_start"]["max"] < 3.0 and 35.0 < s["sweep_ms"]["min"] < 45.0
    for st in res["steps"]:
        assert st["sweep_launches"] == 2 and len(st["rccl"]) == 1 and st["rccl"][0]["end_ms_before_sweep_end"] > 30.0


def test_the_command_line_tools_fail_loudly_on_a_trace_without_steps(tmp_path):
    # a trace whose kernels the tools do not know: non-zero exit, not an empty JSON
    bad = tmp_path / "bad.csv"
    bad.write_text('"Stream_Id","Kernel_Name","Start_Timestamp","End_Timestamp","Workgroup_Size_X","Grid_Size_X"\n"1","k_something_else",0,10,64,64\n')
    for tool in ("overlap_trace.py", "step_timeline.py"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), str(bad)], capture_output=True, text=True)
        assert r.returncode != 0, tool
    ok = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "overlap_trace.py"), TRACE], capture_output=True, text=True)
    assert ok.returncode == 0 and json.loads(ok.stdout)["steps_seen"] == 3
    tl = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "step_timeline.py"), TRACE], capture_output=True, text=True)
    assert tl.returncode == 0
    t = json.loads(tl.stdout)
    assert 40.0 < t["step_ms"] < 45.0 and t["kernels"][0]["kernel"].startswith("k_collide_faces")
    busy = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gpu_busy_from_trace.py"), TRACE, "3"], capture_output=True, text=True)
    assert busy.returncode == 0 and json.loads(busy.stdout)["idle_fraction"] < 0.01


def test_committed_round5_overlap_profiles_are_not_empty():
    """every r05_*_slab_overlap.json under profiles/ saw its steps and says where the exchange ends"""
    prof = os.path.join(ROOT, "profiles")
    files = [f for f in os.listdir(prof) if f.startswith("r05_") and f.endswith("_slab_overlap.json")]
    assert len(files) >= 6
    for f in files:
        d = json.load(open(os.path.join(prof, f)))
        assert d["steps_seen"] >= 5 and d["summary"]["hidden"] is True, f


def test_summarize_profile_arithmetic_on_a_synthetic_profile_directory(tmp_path):
    """tools/summarize_profile.py turns the raw --pmc passes into roofline.traffic and config.step_traffic_bytes.  On a made-up
    profile directory with known numbers: FETCH_SIZE is corrected by the factor the calibration copy yields (2.0 on gfx950: the
    counter tallies 128-byte requests at 64), the mean is over a kernel's LARGEST launches only (the bench runs the same kernels
    on a small replica for its start state), the steady-state sweep is the PULL = true instantiation, and a step's table holds
    the kernels between the last two launches of the sweep times their counter bytes."""
    import summarize_profile as sp

    src, dst = tmp_path / "prof", tmp_path / "out"
    for d in ("trace", "calib_fetch", "calib_write", "pmc_fetch", "pmc_write"):
        (src / d).mkdir(parents=True)
    (src / "trace" / "trace_kernel_stats.csv").write_text('"Name","Calls"\n"x",1\n')
    true_kib = (1 << 30) * 8 / 1024

    def pmc(path, rows):
        with open(path, "w") as f:
            f.write('"Kernel_Name","Grid_Size","Counter_Value"\n')
            for name, grid, val in rows:
                f.write(f'"{name}",{grid},{val}\n')

    copy8, shift = "k_copy8(double const*, double*, unsigned long)", "k_copy8_shift(double const*, double*, unsigned long)"
    pmc(src / "calib_fetch" / "pmc_counter_collection.csv", [(copy8, 1000, true_kib / 2), (shift, 1000, true_kib * 0.75)])
    pmc(src / "calib_write" / "pmc_counter_collection.csv", [(copy8, 1000, true_kib), (shift, 1000, true_kib)])
    sweep = "void ekpnp::k_collide_bulk<4, true, true>(ekpnp::KArgs, int, int, int, int)"
    first = "void ekpnp::k_collide_bulk<4, false, true>(ekpnp::KArgs, int, int, int, int)"
    wall, tri = "void ekpnp::k_collide_wall<4, true, true>(ekpnp::KArgs)", "void ekpnp::k_tridiag_part<8, 64>(ekpnp::PArgs)"
    # sweep: two big launches (mean 100 and 200 KiB raw) and a replica launch that must not count
    pmc(src / "pmc_fetch" / "pmc_counter_collection.csv", [(sweep, 64, 1.0), (sweep, 4096, 90.0), (sweep, 4096, 110.0), (first, 4096, 95.0), (wall, 128, 3.0), (tri, 256, 10.0)])
    pmc(src / "pmc_write" / "pmc_counter_collection.csv", [(sweep, 64, 1.0), (sweep, 4096, 200.0), (sweep, 4096, 200.0), (first, 4096, 200.0), (wall, 128, 2.0), (tri, 256, 11.0)])
    with open(src / "trace" / "trace_kernel_trace.csv", "w") as f:
        f.write('"Stream_Id","Kernel_Name","Start_Timestamp","End_Timestamp","Workgroup_Size_X","Grid_Size_X"\n')
        t = 0
        for name, gx in [(first, 4096), (wall, 128), (tri, 256), (sweep, 64), (sweep, 4096), (wall, 128), (tri, 256), (tri, 256), (tri, 256), ("k_not_profiled()", 8), (sweep, 4096), (wall, 128)]:
            f.write(f'"1","{name}",{t},{t + 5},64,{gx}\n')
            t += 10
    (dst).mkdir()
    json.dump({"cfg2": {"kernel": "kept", "hbm_bytes_per_launch": 1.0}}, open(dst / "pmc_traffic.json", "w"))
    out, bulk, rec = sp.summarize("rXX", "cfg3", str(src), str(dst))
    assert out["calibration"]["fetch_factor"] == 2.0 and out["calibration"]["write_factor"] == 1.0
    assert out["calibration"]["misaligned_by_one_element_fetch_ratio"] == 1.5
    assert bulk == sweep
    assert out["kernels"][sweep]["hbm_read_bytes"] == 100.0 * 1024 * 2.0 and out["kernels"][sweep]["hbm_write_bytes"] == 200.0 * 1024
    assert rec["hbm_bytes_per_launch"] == 400.0 * 1024 and rec["round"] == "rXX"
    table = {e["kernel"]: e for e in rec["step"]["kernels"]}
    assert set(table) == {sweep, wall, tri, "k_not_profiled()"}  # the kernels from the second-to-last big sweep launch up to the last
    assert table[tri]["launches_per_step"] == 3 and table[tri]["hbm_bytes_per_launch"] == (10.0 * 2.0 + 11.0) * 1024
    assert rec["step"]["kernels_without_counters"] == ["k_not_profiled()"]
    assert rec["step"]["hbm_bytes_per_step"] == (400.0 + (3.0 * 2 + 2.0) + 3 * (10.0 * 2 + 11.0)) * 1024
    written = json.load(open(dst / "pmc_traffic.json"))
    assert written["cfg2"]["kernel"] == "kept" and written["cfg3"]["kernel"] == sweep  # other workloads' records stay
    assert os.path.exists(dst / "rXX_cfg3_pmc_summary.json") and os.path.exists(dst / "rXX_cfg3_kernel_stats.csv")
    # bench.py reads the record the same way: a step with a kernel that has no counters yields no step total
    sys.path.insert(0, ROOT)
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_module_for_traffic", os.path.join(ROOT, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.step_traffic_of(rec) is None
    rec["step"]["kernels"] = [e for e in rec["step"]["kernels"] if e["hbm_bytes_per_launch"] is not None]
    rec["step"]["kernels_without_counters"] = []
    assert b.step_traffic_of(rec) == (400.0 + 8.0 + 93.0) * 1024
