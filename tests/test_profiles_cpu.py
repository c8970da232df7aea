"""CPU-side checks of the plane-profile entry points (include/ekpnp.h: ekpnp_plane_sums, ekpnp_stats_*, ekpnp_save_profiles
and their ekpnp_group_* spellings): declared, exported, named consistently in C and Python, and refusing bad arguments with a
status instead of a crash.  No device needed."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = [
    "ekpnp_plane_sums", "ekpnp_stats_reset", "ekpnp_stats_accumulate", "ekpnp_stats_get", "ekpnp_save_profiles",
    "ekpnp_group_plane_sums", "ekpnp_group_stats_reset", "ekpnp_group_stats_accumulate", "ekpnp_group_stats_get",
    "ekpnp_group_save_profiles",
]


def _header_code():
    txt = open(os.path.join(ROOT, "include", "ekpnp.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)  # declarations only, comments stripped


def test_the_ten_entry_points_are_declared_and_exported(pkg):
    code = _header_code()
    lib = pkg.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"include/ekpnp.h does not declare {name}"
        assert hasattr(lib, name), f"libekpnp.so does not export {name}"
        assert name in pkg.exported_symbols()


def test_profile_ids_and_names_agree(pkg):
    code = _header_code()
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(EKPNP_PROF_[A-Z_]+|EKPNP_NPROFILES)\s*=\s*(\d+)", code))
    n = enum.pop("EKPNP_NPROFILES")
    assert n == 24 == len(pkg.PROFILE_NAMES) == len(enum)
    by_id = sorted(enum, key=enum.get)
    assert [enum[k] for k in by_id] == list(range(n))
    # the enum order is the name order ...
    assert [k[len("EKPNP_PROF_"):] for k in by_id] == [name.upper() for name in pkg.PROFILE_NAMES]
    # ... and a field's profile id is its field id
    assert pkg.PROFILE_NAMES[:11] == pkg.FIELDS
    fields = dict((k, int(v)) for k, v in re.findall(r"\b(EKPNP_[A-Z]+)\s*=\s*(\d+)", code) if not k.startswith("EKPNP_PROF_"))
    assert fields.pop("EKPNP_NFIELDS") == 11
    for name, i in pkg.FIELD_ID.items():
        assert fields["EKPNP_" + name.upper()] == i == enum["EKPNP_PROF_" + name.upper()] == pkg.PROFILE_ID[name]


def test_null_arguments_are_refused_not_dereferenced(pkg):
    lib = pkg.load_library()
    buf = (C.c_double * 24 * 8)()
    n = C.c_int(7)
    assert lib.ekpnp_plane_sums(None, buf) == 1  # EKPNP_ERR_INVALID
    assert lib.ekpnp_stats_get(None, buf, C.byref(n)) == 1
    assert lib.ekpnp_group_plane_sums(None, buf) == 1
    assert lib.ekpnp_stats_reset(None) == 1 and lib.ekpnp_stats_accumulate(None) == 1
    assert lib.ekpnp_save_profiles(None, b"/nonexistent/x", 0.0) == 1
    for name in ("ekpnp_group_stats_reset", "ekpnp_group_stats_accumulate"):
        assert getattr(lib, name)(None) == 1
    assert lib.ekpnp_group_stats_get(None, buf, C.byref(n)) == 1
    assert lib.ekpnp_group_save_profiles(None, b"/nonexistent/x", 0.0) == 1


def test_driver_flag_without_a_value_prints_the_usage(pkg):
    exe = os.path.join(ROOT, "ek-pnp-3d_amd", "ekpnp_main")
    assert os.path.exists(exe), "ekpnp_main not built"
    r = subprocess.run([exe, "--profiles-every"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "usage: ekpnp_main" in r.stderr and "--profiles-every N" in r.stderr and "profiles.dat" in r.stderr
