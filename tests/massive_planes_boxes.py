"""The boxes of tests/test_velocity_planes_layout.py and tests/test_velocity_planes_massive_gpu.py: what the velocity planes'
compact layout (massive slots only, tgnh_topology.cpp) can get wrong shows where the massless slot sits in the molecule, how many
there are, and how a box ends.  Built once per name and shared: nobody writes to what box() returns."""
import numpy as np

from openmm_drudenose_amd import synth
from helpers import water_row

# five slots per molecule, one Drude pair (slots 0 and 1), as synth._W_TEST -- with no massless slot, and with two
_W_ALL_MASSIVE = dict(synth._W_TEST, mass=[15.6, 0.4, 1.0, 1.0, 1.0])
_W_TWO_MASSLESS = dict(synth._W_TEST, mass=[15.6, 0.4, 1.0, 0.0, 0.0])

WATER_SIZES = (7, 12, 13, 48, 49, 1001)                                  # molecules; 12 fill a wave tile
ROWS = {"mod2": 48, "mod3": 60, "mod4": 48, "mod5": 60, "mod8": 48, "group-per-tile": 61, "heavy-tiles": 49}   # helpers.WATER_ROWS that qualify
NAMES = ([f"water{n}" for n in WATER_SIZES] + list(ROWS) + ["nacl-order", "all-massive", "two-massless"])
_BOXES = {}


def _from_table(table, n, name):
    rng = np.random.default_rng(synth.SEED)
    mass, pd, pp, resid, pos = synth._molecules(n, table, 0.31)
    return synth._finish(mass, pd, pp, resid, pos, np.zeros(mass.shape[0], np.int32), 1, rng, 300.0, 1.0, name)


def plane_layout(handle):
    """topology(17), taken apart: where the velocity planes keep a massive slot -- word base[tile] + offset[pattern][lane] of each
    plane -> (stride of a plane in words, base[wave tiles + 1], offset[patterns][64]); a box that cannot take the planes: (0, [], [0][64])"""
    a = handle.topology(17).view(np.uint32).astype(np.int64)
    stride, nb = int(a[0]), int(a[1])
    return stride, a[2:2 + nb], a[2 + nb:].reshape(-1, 64)


def box(name):
    """-> (DrudeSystem, group[N], G)"""
    if name not in _BOXES:
        if name.startswith("water"):
            _BOXES[name] = synth.water_box(int(name[5:]))
        elif name in ROWS:
            _BOXES[name] = water_row(name, ROWS[name])
        elif name == "nacl-order":                           # O, H1, H2, M, D: the massless slot fourth of five, the Drude particle behind it
            _BOXES[name] = synth.water_box(49, order="nacl")
        elif name == "all-massive":                          # the compact layout is the identity
            _BOXES[name] = _from_table(_W_ALL_MASSIVE, 49, "all-massive-49")
        elif name == "two-massless":
            _BOXES[name] = _from_table(_W_TWO_MASSLESS, 49, "two-massless-49")
        else:
            raise KeyError(name)
    return _BOXES[name]
