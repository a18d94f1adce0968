"""GPU tests of the nonbonded cell build's other shapes (csrc/tgnh_nonbonded.hip): the states of tests/test_nonbonded_geometry.py --
one cell along every edge with pairs in min_image's division window, a flat box with 1, 2 and 12 cells per edge, cells of exactly
64, 65, 128 and 129 members, 1300 cells under a cutoff of 0.3 nm and a dielectric of 60, and a dielectric of 1 -- in double, mixed
and single precision.  That file asserts the shapes and measures the gate on the CPU.

Tolerances.
 * the force buffer: none.  Every entry changes by the twin's integers, bit for bit; the buffer's total changes by exactly 0 per
   plane; a second call adds the same integers again.
 * the four energies: GEOMETRY_GATE (16 x the margin between twin and reference on these states, 7.2e-14) x the sum of the terms'
   magnitudes, and none of them 0.
 * the counts system with the box changed between calls to one with more cells: that box's own twin, bit for bit."""
import numpy as np
import pytest

from test_nonbonded import PRECISIONS, L, twin_integers, reference_forces
from test_nonbonded_geometry import GEOMETRY, GEOMETRY_GATE, COUNTS_TALL, geometry_state
from test_nonbonded_gpu import context, added_by, set_box

pytestmark = pytest.mark.gpu
_cache = {}


def twin(name, precision):
    if ("twin", name, precision) not in _cache:
        _, x, table, box, _ = geometry_state(name, precision)
        _cache["twin", name, precision] = twin_integers(x, table, box)
    return _cache["twin", name, precision]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", [g for g in GEOMETRY if g != "counts tall"])
def test_geometry_state(name, precision):
    s, x, table, box, info = geometry_state(name, precision)
    ctx, f = context(precision, s, table, box)
    added = added_by(ctx, f, energy=True)
    want = twin(name, precision)
    wrong = np.nonzero((added != want).any(1))[0]
    print(f"{name} {precision}: {len(wrong)} of {ctx.n} slots differ from the twin {wrong[:10]}")
    assert np.array_equal(added, want) and np.any(added != 0)
    assert np.array_equal(added.sum(0), np.zeros(3, np.int64))                   # no reference in this one
    e = f.energy()
    assert ctx.check() == 0
    ref, room = reference_forces(x, table, box)[1:]
    for m, kind in enumerate(("pair Coulomb", "pair LJ", "exception Coulomb", "exception LJ")):
        miss, allowed = float(abs(L(e[m]) - ref[m])), float(L(GEOMETRY_GATE) * room[m])
        print(f"{name} {precision}: {kind} {e[m]:.6f} kJ/mol, off the reference by {miss:.2e}: {miss / allowed:.2f} of what the gate allows ({allowed:.2e})")
        assert miss <= allowed and e[m] != 0
    assert np.array_equal(added_by(ctx, f), want)                                # two calls add twice; the plain launch adds the same
    if name == "counts":
        # the box changed between calls to one with more cells: the per-cell buffers grow
        set_box(ctx, COUNTS_TALL)
        tall = twin("counts tall", precision)
        assert np.array_equal(added_by(ctx, f), tall) and not np.array_equal(tall, want)
        set_box(ctx, box)
        assert np.array_equal(added_by(ctx, f), want)                            # and back
    ctx.close()
