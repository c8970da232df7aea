"""What the CPU and the GPU tests of the tracers' sample share: the numpy transcription of a sample (include/ekpnp.h: the stencil and
the value of tests/_tracers_ref.py on each named array, for q on c - cn formed per node) and eleven random fields per lattice."""
import numpy as np

import _tracers_ref as T

SHAPES = {"W": (70, 66, 13), "O": (35, 33, 5), "R": (40, 12, 17)}
NS = (1, 1000, 4097)
NAMES = ["rho", "c", "cn", "phi", "ux", "uy", "uz", "Ex", "Ey", "Ez", "T", "q"]
VALUE_SETS = {"one": ("T",), "velocity": ("ux", "uy", "uz"), "q": ("q",), "all": tuple(NAMES)}


def all_fields(shape, seed):
    """name -> [nz, ny, nx]: the eleven fields at the sizes a run has (u of 1e-3, E of 1e5, concentrations around 1), read-only"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    scale = {"ux": T.U_SCALE, "uy": T.U_SCALE, "uz": T.U_SCALE, "Ex": T.E_SCALE, "Ey": T.E_SCALE, "Ez": T.E_SCALE, "phi": 0.05}
    out = {}
    for name in NAMES[:11]:
        if name in scale:
            a = scale[name] * rng.uniform(-1.0, 1.0, size=(nz, ny, nx))
        else:
            a = rng.uniform(0.5, 1.5, size=(nz, ny, nx))
        a.setflags(write=False)
        out[name] = a
    return out


def sample(shape, fields, values, x, y, z):
    """[nvalues, n]: the definition, vectorised over the particles; a lost particle gives NaN and reads nothing"""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    lost = np.isnan(x) | np.isnan(y) | np.isnan(z)
    a = np.flatnonzero(~lost)
    st = T._stencil(shape, x[a], y[a], z[a])
    out = np.full((len(values), x.size), np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        for k, name in enumerate(values):
            if name == "q":
                out[k, a] = T._value(fields["c"] - fields["cn"], st)   # the same eight subtractions, made for every node
            else:
                out[k, a] = T._value(fields[name], st)
    return out


def same_sample(got, want):
    """lost particles (NaN in `want`) by isnan, all others by bits"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(T.bits(got)[~nan], T.bits(want)[~nan]))
