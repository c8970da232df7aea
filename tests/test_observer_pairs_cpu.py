"""The schedule of tests/_observer_pairs.py without a device: which pairs it holds, which step count every kind meets, and that
the ring capacities of every configuration make one half of the recorders hold every row and the other half wrap.  Conditions,
not measurements."""
from collections import Counter

import pytest

import _observer_pairs as P

KINDS = P.OBSERVERS + P.MUTATORS


def _kinds(group):
    return [k for k in KINDS if not (group and k in P.GROUP_REFUSED)]


def test_the_kinds_are_the_thirteen_observers_and_seven_mutators():
    assert len(P.OBSERVERS) == 13 and len(P.MUTATORS) == 7 and len(set(KINDS)) == 20
    assert set(P.GROUP_REFUSED) <= set(KINDS) and set(P.RECORDERS) <= set(P.OBSERVERS)
    assert P.K == (1, 2, 5, 4)


def test_every_ordered_observer_pair_appears_exactly_once():
    pairs = Counter((x, y) for _, x, y in P.schedule() if x in P.OBSERVERS and y in P.OBSERVERS)
    assert len(pairs) == 169 and set(pairs.values()) == {1}
    assert set(pairs) == {(x, y) for x in P.OBSERVERS for y in P.OBSERVERS}


def test_every_observer_mutator_pair_appears_exactly_once_in_either_order():
    s = P.schedule()
    assert len(s) == 169 + 182
    om = Counter((x, y) for _, x, y in s if x in P.OBSERVERS and y in P.MUTATORS)
    mo = Counter((x, y) for _, x, y in s if x in P.MUTATORS and y in P.OBSERVERS)
    assert set(om) == {(x, y) for x in P.OBSERVERS for y in P.MUTATORS} and set(om.values()) == {1}
    assert set(mo) == {(x, y) for x in P.MUTATORS for y in P.OBSERVERS} and set(mo.values()) == {1}
    assert not [t for t in s if t[1] in P.MUTATORS and t[2] in P.MUTATORS]   # mutator pairs are tests/diagnostics/api_fuzz.py's


@pytest.mark.parametrize("group", [False, True])
def test_k_cycles_and_consecutive_triples_do_not_share_their_first_operation(group):
    s = P.schedule(group)
    assert [k for k, _, _ in s] == [P.K[i % 4] for i in range(len(s))]
    assert all(a[1] != b[1] for a, b in zip(s, s[1:]))


@pytest.mark.parametrize("group", [False, True])
def test_every_kind_follows_each_step_count(group):
    s = P.schedule(group)
    for kind in _kinds(group):
        assert {k for k, x, _ in s if x == kind} == set(P.K), kind


@pytest.mark.parametrize("group", [False, True])
def test_every_kind_is_the_last_operation_before_a_step_of_five_and_of_one(group):
    s = P.schedule(group)
    for kind in _kinds(group):
        after = {nxt[0] for cur, nxt in zip(s, s[1:]) if cur[2] == kind}
        assert {5, 1} <= after, (kind, after)


def test_the_group_schedule_holds_no_refused_kind_and_otherwise_the_same_pairs():
    single, group = P.schedule(False), P.schedule(True)
    assert not [t for t in group if t[1] in P.GROUP_REFUSED or t[2] in P.GROUP_REFUSED]
    kept = Counter((x, y) for _, x, y in single if x not in P.GROUP_REFUSED and y not in P.GROUP_REFUSED)
    assert Counter((x, y) for _, x, y in group) == kept and set(kept.values()) == {1}
    assert len(group) == 11 * 11 + 2 * 11 * 6


def test_the_schedule_is_the_same_list_every_time():
    assert P.schedule() == P.schedule() and P.schedule(True) == P.schedule(True)


@pytest.mark.parametrize("name", list(P.CONFIGS))
def test_ring_capacities_hold_every_row_or_wrap_many_times(name):
    cfg = P.CONFIGS[name]
    s = P.schedule(cfg["nslabs"] > 1)
    rows, cap = P.rows_recorded(cfg, s), P.capacities(cfg, s)
    assert set(rows) == set(cap) == set(P.recorders(cfg))
    for r in rows:
        if r in P.HALVES[cfg["big"]]:
            assert rows[r] <= cap[r], r   # every row is held and compared
        else:
            assert cap[r] == 4 and rows[r] > 8, r   # the ring really wraps
    assert P.settled_index(s) < len(s) // 2   # most of the schedule runs under the no-allocation check


def test_the_halves_swap_between_configurations():
    assert sorted(P.HALVES[0] + P.HALVES[1]) == sorted(P.RECORDERS)
    for family in (False, True):
        cfgs = [c for c in P.CONFIGS.values() if (c["nslabs"] > 1) == family]
        for r in P.recorders(cfgs[0]):
            held = [r in P.HALVES[c["big"]] for c in cfgs]
            assert any(held) and not all(held), r   # fully checked in one configuration, wrapping in another


@pytest.mark.parametrize("name", list(P.CONFIGS))
def test_the_library_accepts_the_specs_of_every_configuration(pkg, name):
    """host arithmetic only: the spec checks of include/ekpnp.h need no device"""
    cfg = P.CONFIGS[name]
    p = P.params(pkg, cfg)
    planes = P.planes_of(cfg)
    pkg.modes_spec_check(p, pkg.modes_spec("uz", P.TRACK))
    pkg.spectrum_spec_check(p, pkg.spectrum_spec("uz", planes))
    values, across, rng, _ = P.section_args(cfg)
    pkg.section_spec_check(p, pkg.section_spec(values, across, rng, planes))
    pkg.hist_spec_check(p, pkg.hist_spec(("q", 24, -1.0, 1.0), (cfg["second"], 6, -1.0, 1.0)), planes=P.hist_planes_of(cfg), capacity=4)
    pkg.monitor_spec_check(P.monitor_quantities(pkg, cfg), cfg["every"], 4)
    X, Y, Z, _ = pkg.snapshot_extent(p, P.SNAP_FIELDS, P.snap_coarsen(cfg))
    assert Z == p.nz and X * P.snap_coarsen(cfg)[0] == p.nx and Y * P.snap_coarsen(cfg)[1] == p.ny
    if cfg["nslabs"] == 1:
        spec = pkg.tracers_spec_check(p, P.tracers_spec(pkg, cfg))
        assert 200 <= spec.n <= 999
    else:
        cuts = [pkg.slab_extent(p.nz, r, cfg["nslabs"]) for r in range(cfg["nslabs"])]
        if name == "G3-inplace":   # uneven slabs, and only one of them owns the chosen plane and the histogram range
            assert sorted(n for _, n in cuts) == [5, 6, 6]
            assert sum(z0 <= planes[0] < z0 + n for z0, n in cuts) == 1 and planes == [6] and P.hist_planes_of(cfg) == (6, 6)
