"""GPU tests of the library's DrudeForce, bonded forces and NonbondedForce past one trip of the grid-stride loop and with more than
256 rows of energy: the systems of tests/test_library_forces_at_size.py, which asserts their shapes and derives the depth of the
energy sums on the CPU.

Tolerances: each unit's own, from its own test file.
 * DrudeForce: a slot that receives isotropic shares only -- all but the 20 sites of the five screened pairs -- changes by the numpy
   restatement's integers, bit for bit; a site of a screened pair within tests/test_drude_force.py's GATE per contribution.
 * bonded: the bond shares as the twin's integers and per contribution of an angle or a torsion tests/test_bonded_forces.py's GATE x
   the term's uncancelled scale x 2^32 plus one unit, as tests/test_bonded_forces_gpu.py has it (the device's atan2 is not numpy's:
   a slot with an angle share cannot be asked for the twin's bits); a slot with bond shares only: the twin's integers.
 * nonbonded: none.  Every entry changes by the twin's integers, and the buffer's total by exactly 0 per plane.
 * every energy: (the unit's GATE + sum_depth x 2^-53) x the sum of the terms' magnitudes, against the fp80 sum.
Each test prints its wall time and the energy's miss as a share of its gate."""
import time

import numpy as np
import pytest

from openmm_drudenose_amd.drudetgnhplugin import HipContext
from openmm_drudenose_amd.forces import BondedForces
import test_bonded_forces as tb
import test_drude_force as td
import test_nonbonded as tn
from test_bonded_forces_gpu import snapshot, planes
from test_drude_force_gpu import K3
from test_library_forces_at_size import (NB_BOX, bonded_at_size, drude_at_size, nonbonded_at_size, nonbonded_pairs, sum_depth, trips)
from test_nonbonded_geometry import index_grid, nb_pair_grid
from test_nonbonded_gpu import context as nonbonded_context, added_by

pytestmark = pytest.mark.gpu
L, FIXED, EPS = np.longdouble, 4294967296.0, 2.0 ** -53


def stored_positions(ctx, s, precision):
    """the positions as the context stores them; they are the stored types' reading of the system's"""
    x = ctx.getPositions()
    assert np.array_equal(x, tn.stored(s.positions, precision)["x"])
    return x


def split(ref, twin, n, exact_kind, gate, scale_of):
    """tests/test_*_gpu.py's `expected`: -> (exact [n, 3] int64 from the twin's shares of `exact_kind`; near [n, 3] fp80: every other
    share x 2^32 from the reference; tol [n, 3]: what the gate allows; count [n]: conversions per slot)"""
    exact, near, tol, count = np.zeros((n, 3), np.int64), np.zeros((n, 3), L), np.zeros((n, 3), L), np.zeros(n, np.int64)
    for r, t in zip(ref, twin):
        scale = scale_of(r)
        for s, rs, ts in zip(r[1], r[2], t[2]):
            np.add.at(count, s, 1)
            if r[0] == exact_kind:
                np.add.at(exact, s, np.rint(ts * FIXED).astype(np.int64))
            else:
                np.add.at(near, s, rs * L(FIXED))
                np.add.at(tol, s, np.broadcast_to(L(gate) * scale * L(FIXED) + 1, rs.shape))
    return exact, near, tol, count


def report(what, e, want, room, gate, depth, t0=None):
    """the energies against the fp80 sums: (gate + depth x 2^-53) x the sum of the terms' magnitudes; prints each miss as a share of it"""
    for name, got, w, r in zip(what, e, want, room):
        miss, allowed = float(abs(L(got) - w)), float((L(gate) + depth * L(EPS)) * r)
        print(f"at size, {name}: {got:.6f} kJ/mol, off the fp80 sum by {miss:.2e}: {miss / allowed:.4f} of the gate ({allowed:.2e}; depth {depth})")
        assert miss <= allowed and got != 0
    if t0 is not None:
        print(f"at size, {what[0].split()[0]}: {time.perf_counter() - t0:.1f} s of wall time")


@pytest.mark.parametrize("precision", td.PRECISIONS)
def test_drude_force_past_one_trip(precision):
    t0 = time.perf_counter()
    s = drude_at_size()
    tables = s.drude_force.tables()
    n = s.num_particles
    ctx = HipContext(s, td.integrator(), mode="TGNH", precision=precision)
    ctx.force.zero_()
    ctx.compute_drude_force(energy=True)
    e = ctx.drude_energy()
    assert ctx.check() == 0
    x = stored_positions(ctx, s, precision)
    got = planes(snapshot(ctx)["force"], ctx)
    ref, twin = td.evaluate(tables, x, L), td.evaluate(tables, x, np.float64)
    exact, near, tol, count = split(ref, twin, n, "isotropic", td.GATE, lambda r: np.max([np.abs(v).max(1) for v in r[2]], axis=0)[:, None])
    pure, gated = (count > 0) & (tol[:, 0] == 0), tol[:, 0] > 0
    assert gated.sum() == 20 and pure.sum() == n - 3 - 20 and gated[1024 * 256:].any()          # (five screened pairs of four sites, none shared)
    # the numpy restatement of the springs, three lines: the same integers as the twin's, and the device's
    t = K3 * (x[s.pair_drude] - x[s.pair_parent])
    three_lines = np.zeros((n, 3), np.int64)
    three_lines[s.pair_drude], three_lines[s.pair_parent] = np.rint(-t * FIXED).astype(np.int64), np.rint(t * FIXED).astype(np.int64)
    assert np.array_equal(three_lines, exact)
    wrong = np.nonzero((got != exact).any(1) & pure)[0]
    print(f"at size, DrudeForce {precision}: {len(wrong)} of {pure.sum()} isotropic slots differ from the restatement {wrong[:8]}")
    assert np.array_equal(got[pure], exact[pure]) and np.any(got[1024 * 256:n - 3] != 0)
    miss = np.abs((got - exact).astype(L) - near)
    assert np.all(miss <= tol)
    assert np.array_equal(got[count == 0], np.zeros((3, 3), np.int64)) and np.abs(got.sum(0)).max() <= 0.5 * count.sum()
    # the energies: a thread adds one row's springs a trip, and up to one screened pair a receiver
    recv = 2 * len(tables[0])
    depth = sum_depth(trips(recv) * 1, index_grid(recv))
    room = [sum(np.abs(t[3]).sum() for t in ref if t[4] == scr) for scr in (False, True)]
    report((f"DrudeForce {precision} springs", f"DrudeForce {precision} screened pairs"), e, td.energies(ref), room, td.GATE, depth, t0)
    ctx.close()


def test_bonded_forces_past_one_trip():
    t0 = time.perf_counter()
    precision = "mixed"
    s, tables = bonded_at_size()
    n = s.num_particles
    ctx = HipContext(s, tb.integrator(), mode="TGNH", precision=precision)
    f = BondedForces(ctx, *tables)
    assert f.num_terms == tuple(len(t[0]) for t in tables)
    ctx.force.zero_()
    f.compute(energy=True)
    e = f.energy()
    assert ctx.check() == 0
    x = stored_positions(ctx, s, precision)
    got = planes(snapshot(ctx)["force"], ctx)
    ref, twin = tb.evaluate(tables, x, L), tb.evaluate(tables, x, np.float64)
    exact, near, tol, count = split(ref, twin, n, "bond", tb.GATE, lambda r: r[4][:, None])
    pure, gated = (count > 0) & (tol[:, 0] == 0), tol[:, 0] > 0
    recv = tb.receivers(tables)
    assert np.array_equal(np.flatnonzero(count > 0), recv) and pure.sum() == 6 * 490 and trips(len(recv)) == 2
    assert np.array_equal(got[pure], exact[pure]) and np.any(got[pure] != 0)
    miss = np.abs((got - exact).astype(L) - near)
    late = recv[1024 * 256:]                                     # the receivers of the second trip
    print(f"at size, bonded {precision}: largest miss {float((miss[gated] / tol[gated]).max()):.2e} of what the gate allows; {len(late)} receivers in the second trip, "
          f"{np.count_nonzero((got[late] != 0).any(1))} of them with a force")
    assert np.all(miss <= tol)
    assert np.count_nonzero((got[late] != 0).any(1)) > 0.9 * len(late)
    assert np.array_equal(got[count == 0], np.zeros_like(got[count == 0])) and np.abs(got.sum(0)).max() <= 0.5 * count.sum()
    # the energies: a thread adds, per trip, the terms its receiver is p1 of -- at most the entries of the busiest receiver
    depth = sum_depth(trips(len(recv)) * int(count.max()), index_grid(len(recv)))
    room = [np.abs(t[3]).sum() for t in ref]
    report(tuple(f"bonded {precision} {k}s" for k in tb.KINDS), e, tb.energies(ref), room, tb.GATE, depth, t0)
    ctx.close()


def test_nonbonded_force_past_one_trip():
    t0 = time.perf_counter()
    precision = "mixed"
    s, table = nonbonded_at_size()
    n = s.num_particles
    pairs, gap = nonbonded_pairs(precision)
    assert gap >= 1e-9
    x = tn.stored(s.positions, precision)["x"]
    want = tn.twin_integers(x, table, NB_BOX, pairs)
    ctx, f = nonbonded_context(precision, s, table, NB_BOX)
    assert f.num_terms == (n, n // 2, n // 2)
    added = added_by(ctx, f, energy=True)
    e = f.energy()
    assert ctx.check() == 0
    wrong = np.nonzero((added != want).any(1))[0]
    print(f"at size, nonbonded {precision}: {len(wrong)} of {n} slots differ from the twin {wrong[:8]}")
    assert np.array_equal(added, want) and np.any(added[1024 * 256:] != 0)
    assert np.array_equal(added.sum(0), np.zeros(3, np.int64))
    # the fp80 energies over the same pair list, each pair once; the exceptions from their first receiver
    once = pairs[0] < pairs[1]
    p, x80 = tn.pair_terms(x, table, NB_BOX, L, (pairs[0][once], pairs[1][once])), tn.exception_terms(x, table, L)
    assert len(p["a"]) == len(tn.pair_terms(x, table, NB_BOX, np.float64, (pairs[0][once], pairs[1][once]))["a"])        # the same pairs in both
    first = x80["role"] == 0
    terms = (p["e_c"], p["e_lj"], x80["e_c"][first], x80["e_lj"][first])
    # a lane of the pair launch adds its neighbours of a larger slot; an exception receiver adds one row a trip
    ncells = int(np.prod(tn.cells_per_edge(NB_BOX, table[1])))
    depth_pairs = sum_depth(int(np.bincount(p["a"], minlength=n).max()), nb_pair_grid(n, ncells))
    depth_exc = sum_depth(trips(2 * (n // 2)) * 1, index_grid(2 * (n // 2)))
    report((f"nonbonded {precision} pair Coulomb", f"nonbonded {precision} pair LJ"), e[:2], [t.sum() for t in terms[:2]], [np.abs(t).sum() for t in terms[:2]],
           tn.GATE, depth_pairs)
    report((f"nonbonded {precision} exception Coulomb", f"nonbonded {precision} exception LJ"), e[2:], [t.sum() for t in terms[2:]],
           [np.abs(t).sum() for t in terms[2:]], tn.GATE, depth_exc, t0)
    ctx.close()
