"""The CPU oracle satisfies the two exact properties of tests/_equivariance.py - x-y shift equivariance and one-link locality of
init_equilibrium + k calls of stream_collide_save with E held in its arrays - on every case of the shared list.  That shows
that the properties belong to the operation (not to one implementation of it) and that the start states are valid inputs;
and since tests/test_equivariance_gpu.py asserts them of the HIP path with the same helpers, a mistake in a helper or in a
case fails here first.  Knobs that exist only in the product (launch shapes, z slabs) are ignored.  No tolerance anywhere."""
import functools

import pytest

import _equivariance as EQ


@functools.lru_cache(maxsize=2)
def _setup(O, case_id):
    """(params, start, plain run) of a case: computed once, shared by its shift and its locality test, never changed"""
    case = EQ.CASES[EQ.CASE_IDS.index(case_id)]
    po = EQ.case_params(O, case)
    start = EQ.start_state(O, po, seed=EQ.CASE_IDS.index(case_id))
    return po, start, EQ.run(EQ.OracleEngine(O), po, None, start, EQ.SHIFT_CALLS)


@pytest.mark.parametrize("case_id", EQ.CASE_IDS)
def test_oracle_commutes_with_xy_shifts(O, case_id):
    case = EQ.CASES[EQ.CASE_IDS.index(case_id)]
    po, start, plain = _setup(O, case_id)
    shifts = EQ.case_shifts(case)
    assert shifts
    for shift in shifts:
        EQ.check_shift(EQ.OracleEngine(O), po, None, start, shift, EQ.SHIFT_CALLS, plain=plain)


@pytest.mark.parametrize("case_id", EQ.CASE_IDS)
def test_oracle_one_node_change_stays_in_its_ball(O, case_id):
    case = EQ.CASES[EQ.CASE_IDS.index(case_id)]
    po, start, plain = _setup(O, case_id)
    for node, field in EQ.case_locality(case):
        EQ.check_locality(EQ.OracleEngine(O), po, None, start, node, field, EQ.LOCALITY_CALLS, plain=plain)


def test_case_list_reaches_what_it_names():
    """the case data itself: the tile arithmetic the table of cases promises, shifts distinct modulo the lattice, every
    locality node inside the lattice, both sides of every slab seam present, unequal slabs with one of four planes"""
    by_id = {c["id"]: c for c in EQ.CASES}
    assert by_id["64x3x6"]["shape"][0] % 64 == 0 and by_id["130x4x8"]["shape"][0] % 64 == 2 and by_id["70x5x9"]["shape"][0] % 64 == 6
    assert EQ.case_shifts(by_id["2x2x5"]) == [(1, 0), (0, 1), (1, 1)]
    assert EQ.case_shifts(by_id["64x3x6"]) == [(1, 0), (0, 1), (63, 2)]
    assert EQ.case_shifts(by_id["130x4x8"]) == [(1, 0), (0, 1), (129, 3), (63, 1), (64, 3)]
    heights = set()
    for c in EQ.CASES:
        nx, ny, nz = c["shape"]
        nodes = EQ.case_locality(c)
        assert all(0 <= z < nz and 0 <= y < ny and 0 <= x < nx for (z, y, x), _ in nodes)
        zs = [n[0] for n, _ in nodes]
        assert {0, 1, nz - 1} <= set(zs) and any(n[2] == 0 and n[1] == ny - 1 and 0 < n[0] < nz - 1 for n, _ in nodes)
        assert nx <= 64 or any(n[2] == 64 for n, _ in nodes)
        n = c.get("knobs", {}).get("nslabs", 1)
        edges = [0] + EQ.slab_seams(nz, n) + [nz]
        for z0 in edges[1:-1]:
            assert z0 - 1 in zs and z0 in zs
        if n > 1:
            h = [b - a for a, b in zip(edges, edges[1:])]
            assert len(set(h)) > 1 and min(h) >= 4
            heights |= set(h)
    assert 4 in heights
