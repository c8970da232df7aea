"""GPU tests of the on-device diagnostics TOGETHER (tests/_observer_pairs.py has the schedule and the three twins).

1. One test per configuration: every ordered pair of the thirteen observers and every observer / mutator pair in either order,
   as `step(k); X; Y`, on a twin A with every ring armed, a twin B that only makes synchronous calls and a twin C that is only
   stepped.  Every ring row, running profile, snapshot file, field, checkpoint and tracer is compared bit for bit (the sums of a
   SORTED cloud's moments within the bound of tests/test_tracers_sort_gpu.py:221-235, see the helper's docstring).
2. The driver with every diagnostics flag at once: each file it writes is byte for byte the file of a run with that flag alone, the
   end state is the one of a run without any of them, and --batch 1 writes what --batch 0 writes.  A group's solve rounds phi
   differently from a single context's (tests/test_group_gpu.py), so the end states are compared within the single-context
   runs and within the group runs."""
import os
import time

import pytest

import _observer_pairs as P
from test_hist_gpu import _run_driver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")


# ---- 1. the schedule on three twins ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(P.CONFIGS))
def test_observers_change_neither_the_run_nor_each_other(pkg, name, tmp_path):
    t0 = time.perf_counter()
    out = P.run(pkg, name, tmp_path)
    print(f"{name}: {time.perf_counter() - t0:.2f} s, {out}")
    cfg = P.CONFIGS[name]
    full = P.schedule(cfg["nslabs"] > 1)
    assert out["triples"] == len(full) and out["steps"] == sum(k for k, _, _ in full)
    assert out["rows"] == P.rows_recorded(cfg, full) and out["snapshots"] == 2 * (len(P.OBSERVERS) - (2 if cfg["nslabs"] > 1 else 0)) + 2 * (len(P.MUTATORS) - (1 if cfg["nslabs"] > 1 else 0))
    # the run the observers looked at is a run: finite, moving, with a field between the plates and a cloud that is still there
    assert out["nonfinite"] == 0, out["largest"]
    assert out["largest"]["uz"] > 0.0 and out["largest"]["Ex"] > 0.0 and out["largest"]["phi"] > 0.0
    if cfg["nslabs"] == 1:
        assert out["alive"] > 0


# ---- 2. the driver: all flags at once ---------------------------------------------------------------------------------------

GEO = ["--nx", "40", "--ny", "12", "--nz", "17", "--steps", "12", "--seed-pattern", "squares", "--seed-modes", "1,1", "--binary-state", "1"]
GROUP = ["--devices", "0,0,0"]
# flag -> (its options, the files it writes)
FLAGS = {
    "monitor": (["--monitor-every", "3"], ["monitor.dat"]),
    "modes": (["--modes-every", "2"], ["modes.dat"]),
    "spectrum": (["--spectrum-every", "4"], ["spectrum.dat"]),
    "hist": (["--hist-every", "3", "--hist-value", "q", "--hist-bins", "24", "--hist-range", "-0.5,0.5", "--hist-value2", "Ex", "--hist-bins2", "6",
              "--hist-range2", "-1e5,1e5"], ["hist.dat"]),
    "section": (["--section-every", "2", "--section-full-every", "4", "--section-values", "phi,q,uz"],
                ["section.dat", "section_0000004.dat", "section_0000008.dat", "section_0000012.dat"]),
    "profiles": (["--profiles-every", "3"], ["profiles.dat"]),
    "snap": (["--snap-every", "4", "--snap-coarsen", "2,2,1", "--snap-fields", "uz,Ex"], ["snap_0000004.vtk", "snap_0000008.vtk", "snap_0000012.vtk"]),
    "tracers": (["--tracers-grid", "8,6,5", "--tracers-every", "2", "--tracers-sort-every", "2", "--tracers-mobility", "1e-9"], ["tracers.dat", "tracers_final.bin"]),
}
PLAIN = ["data.dat", "umax.dat", "data_end.dat", "data_end.bin"]   # what a run without any of the flags writes
FAMILIES = {"one": [], "group": GROUP}


def _flags_of(family):
    return [f for f in FLAGS if not (family == "group" and f == "tracers")]   # the driver refuses tracers on a group


@pytest.fixture(scope="module")
def all_at_once(pkg, tmp_path_factory):
    """per family: the run without any diagnostics flag and the runs with all of them, --batch 0 and --batch 1 (one child at a time)"""
    assert os.path.exists(EXE), "ekpnp_main not built"
    tmp = tmp_path_factory.mktemp("driver_all")
    runs, seconds = {}, {}
    for family, extra in FAMILIES.items():
        every = [opt for f in _flags_of(family) for opt in FLAGS[f][0]]
        for tag, args in (("plain", []), ("batch0", [*every, "--batch", "0"]), ("batch1", [*every, "--batch", "1"])):
            t0 = time.perf_counter()
            runs[family, tag], _ = _run_driver([*GEO, *extra, *args], tmp / f"{family}_{tag}")
            seconds[family, tag] = round(time.perf_counter() - t0, 2)
    print(f"driver, all flags at once: {seconds}")
    return runs


@pytest.mark.parametrize("family", list(FAMILIES))
def test_driver_with_every_flag_writes_every_file_and_batch_changes_none(all_at_once, family):
    plain, b0, b1 = (all_at_once[family, t] for t in ("plain", "batch0", "batch1"))
    want = sorted(PLAIN + [f for fl in _flags_of(family) for f in FLAGS[fl][1]])
    assert sorted(os.listdir(plain)) == sorted(PLAIN)
    assert sorted(os.listdir(b0)) == want and sorted(os.listdir(b1)) == want
    for f in want:
        x = (b0 / f).read_bytes()
        assert len(x) > 0 and x == (b1 / f).read_bytes(), (family, f)
    for f in PLAIN:   # the diagnostics leave the run alone: the end state and the reference's own files are the plain run's
        assert (b0 / f).read_bytes() == (plain / f).read_bytes(), (family, f)


@pytest.mark.parametrize("family, flag", [(fam, fl) for fam in FAMILIES for fl in FLAGS if not (fam == "group" and fl == "tracers")])
def test_driver_file_of_a_flag_is_the_file_of_that_flag_alone(all_at_once, tmp_path, family, flag):
    t0 = time.perf_counter()
    alone, _ = _run_driver([*GEO, *FAMILIES[family], *FLAGS[flag][0], "--batch", "0"], tmp_path / "alone")
    print(f"driver, {family}, {flag} alone: {time.perf_counter() - t0:.2f} s")
    together, plain = all_at_once[family, "batch0"], all_at_once[family, "plain"]
    assert sorted(os.listdir(alone)) == sorted(PLAIN + FLAGS[flag][1])
    for f in FLAGS[flag][1]:
        x = (alone / f).read_bytes()
        assert len(x) > 0 and x == (together / f).read_bytes(), (family, flag, f)
    for f in PLAIN:
        assert (alone / f).read_bytes() == (plain / f).read_bytes(), (family, flag, f)
