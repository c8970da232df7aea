"""The collide sweep of the HIP path, node by node and bit by bit: the two exact properties of tests/_equivariance.py.

Every other comparison of the collide kernels goes through one global rel-L2 number per field group, taken over fields with
large means (rho ~ 1000, c ~ 0.01, T): it does not see an error at a few nodes, and it does not single out the nodes the
code treats specially - the last, partially filled 64-node tile of a row and its pad lanes, the x and y wrap, the dense halo
planes the edge kernels read, the rows a rounded-up grid launches beyond the last one, the y-band order.  Here

1. init_equilibrium + 0 .. 3 calls of stream_collide_save commute bit for bit with a periodic x-y roll of all eleven input
   fields, in every field and every population of every lattice (read from a whole-lattice checkpoint): shifts by one node
   in x, in y, by (nx - 1, ny - 1) and, where a row has more than one tile, by (63, 1) and (64, ny - 1), which move every
   node to another lane and to another tile;
2. a change of one field at one node is, after 1 and after 2 calls, visible at that node and nowhere outside the periodic
   Chebyshev ball of radius 1 and 2 around it: a store that lands elsewhere, or a load from a wrong neighbour, shows.

The cases (tests/_equivariance.py: CASES) are the smallest shapes at which each launch path still runs: the merged kernel, the
separate bulk and wall kernels, the ordered in-place sweep, one and three lattices, moving wall and body force, y bands,
and z slabs of unequal height down to four planes, in place and not.  tests/test_equivariance_cpu.py asserts the same of the
CPU oracle with the same helpers.  Every assertion is np.array_equal or set inclusion; there is no tolerance.

NOT covered: the EPHI instantiations, which form E from the phi the last solve left.  A rolled input does not reach them bit
for bit, because the Poisson solve commutes with a shift only to rounding (phi to 7e-16, E to 1e-12 on the oracle), so the
properties are asked of the collide with E set from outside (test_lazy_efield_gpu.py::test_fields_set_from_outside_are_honoured:
that E is what the collide reads).  The EPHI variants stay tied to the ones tested here by
test_lazy_efield_gpu.py::test_lazy_efield_is_bitwise_the_eager_path, bitwise at every node, on the shapes of this list."""
import pytest

import _equivariance as EQ

pytestmark = pytest.mark.gpu

_CACHE = {}


def _setup(pkg, O, case_id):
    """(case, params, knobs, start, plain run, hook): computed once per case, shared by its two tests, never changed"""
    if _CACHE.get("id") != case_id:
        case = EQ.CASES[EQ.CASE_IDS.index(case_id)]
        p = EQ.case_params(pkg, case)
        start = EQ.start_state(O, EQ.case_params(O, case), seed=EQ.CASE_IDS.index(case_id))
        knobs = case.get("knobs", {})

        def hook(e, want=case.get("band_rows")):
            if want is not None:
                assert e.s.pass_order()["band_rows"] == want

        plain = EQ.run(EQ.ProductEngine(pkg), p, knobs, start, EQ.SHIFT_CALLS, after_create=hook)
        _CACHE.clear()
        _CACHE.update(id=case_id, value=(case, p, knobs, start, plain))
    return _CACHE["value"]


@pytest.mark.parametrize("case_id", EQ.CASE_IDS)
def test_collide_commutes_with_xy_shifts(pkg, O, case_id):
    case, p, knobs, start, plain = _setup(pkg, O, case_id)
    for shift in EQ.case_shifts(case):
        EQ.check_shift(EQ.ProductEngine(pkg), p, knobs, start, shift, EQ.SHIFT_CALLS, plain=plain)


@pytest.mark.parametrize("case_id", EQ.CASE_IDS)
def test_one_node_change_stays_in_its_ball(pkg, O, case_id):
    case, p, knobs, start, plain = _setup(pkg, O, case_id)
    for node, field in EQ.case_locality(case):
        EQ.check_locality(EQ.ProductEngine(pkg), p, knobs, start, node, field, EQ.LOCALITY_CALLS, plain=plain)
