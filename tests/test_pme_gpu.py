"""GPU tests of smooth particle-mesh Ewald on the library's NonbondedForce (csrc/tgnh_pme.hip; tgnh_set_nonbonded_pme,
tgnh_get_pme_grids, forces.NonbondedForces).  The states, the fp80 reference, its fp64 twin and the gate are those of
tests/test_pme.py, which holds the reference to the explicit Ewald sum and to finite differences of its own energy, and measures
the gate on the CPU.

Tolerances.
 * exact: the int64 charge grid equals the twin's, bit for bit, on every state (B-splines need no math library, integer adds commute);
   reversed molecules give the same grid, the same phi bits and the permuted force bits; twice, from another handle, replayed from
   a graph: the same bits; all charges 0: the reaction-field call's bits; after tgnh_set_nonbonded_force: tests/test_nonbonded.py's twin.
 * phi on the transform-only grids: GATE_PME x Phi_abs, the absolute value of the real-space kernel convolved with |Q| -- Q being
   exact, this checks the transform and the influence function alone.
 * forces, per slot and component: GATE_PME x S_i plus 2^-33 per converted contribution of the slot (force_gate); the eight energies:
   GATE_PME x the sum of the terms' magnitudes, each."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import _lib
from openmm_drudenose_amd.drudetgnhplugin import TgnhError, FLAG_GATHER
from openmm_drudenose_amd.forces import NonbondedForces
from test_nonbonded import PRECISIONS, FIXED, K, L, BOX_B, BOX_B_MORE, system_a, system_b
from test_nonbonded_gpu import context, added_by, set_box, twin, reversed_molecules
from test_bonded_forces_gpu import bits, snapshot, planes
from test_ewald import ENERGIES, MADELUNG, ROCK_A, rock_salt, lattice_e4, charged_b, ewald_b
from test_pme import (GATE_PME, THIN_GRIDS, MIXED_GRIDS, GRID_P2, pme_states, pme_evaluated, force_gate, phi_state, phi_checked, pdesc)

pytestmark = pytest.mark.gpu
SYSTEMS = {"P1": lambda: rock_salt()[0], "P2": lambda: system_b()[0], "P3": lambda: system_a()[0], "P4": lambda: lattice_e4()[0]}


def pme_context(name, precision, mode="TGNH", flags=0):
    """a context over the state's system with PME on -> (ctx, the NonbondedForces on it)"""
    x, table, box, pme = pme_states()[name, precision]
    ctx, f = context(precision, SYSTEMS[name[:2]](), table, box, mode, flags, x=x)
    f.set_pme(*pme)
    assert f.pme == (pme[0], tuple(pme[1:])) and f.ewald is None
    return ctx, f


def check_state(name, precision, ctx, f):
    """one want_energy call: the charge grid against the twin, forces and the eight energies against the reference"""
    added = added_by(ctx, f, energy=True)
    ref = pme_evaluated(name, precision, L)
    Q, phi = f.pme_grids()
    assert Q.dtype == np.int64 and np.array_equal(Q, pme_evaluated(name, precision, np.float64)["Q"]) and np.any(Q != 0)
    off = np.abs(added.astype(L) / L(FIXED) - ref["force"])
    gate = force_gate(ref)
    print(f"{name} {precision}: forces off the reference by at most {float((off / np.maximum(gate, L(1e-300))).max()):.3f} of the gate; "
          f"largest force {float(np.abs(ref['force']).max()):.1f} kJ/mol/nm, largest deviation {float(off.max()):.2e}; "
          f"phi off by {float((np.abs(phi.astype(L) - ref['phi']) / ref['phi_abs']).max()):.2e} of Phi_abs")
    assert np.all(off <= gate)
    assert np.all(np.abs(phi.astype(L) - ref["phi"]) <= L(GATE_PME) * ref["phi_abs"])
    e = f.energy() + f.ewald_energy()
    for m, kind in enumerate(ENERGIES):
        d, room = abs(L(e[m]) - ref["energy"][m]), L(GATE_PME) * ref["mag"][m]
        print(f"{name} {precision}: {kind} {e[m]:.6f} kJ/mol, off the reference by {float(d):.2e}, the gate allows {float(room):.2e}")
        assert d <= room
    return added, e, ref


@pytest.mark.parametrize("precision", PRECISIONS)
def test_p1_rock_salt(precision):
    """64 ions, an ion at s = 0 exactly; the total against the Madelung energy is a record of the mesh's error at this grid"""
    ctx, f = pme_context("P1", precision)
    added, e, ref = check_state("P1", precision, ctx, f)
    want = -L(32) * L(MADELUNG) * L(K) / L(ROCK_A / 2)
    print(f"rock salt {precision}, grid {f.pme[1]}: total {float(sum(L(v) for v in e)):.9f} against the Madelung energy {float(want):.9f}")
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_p2_system_b_with_a_net_charge(precision):
    """exclusions, evaluated exceptions, molecules two box lengths outside, three grid sizes with all three radices, a net charge"""
    ctx, f = pme_context("P2", precision)
    assert ctx.padded > ctx.n
    added, e, _ = check_state("P2", precision, ctx, f)
    assert all(v != 0 for v in e) and e[6] < -1e-3
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_p3_the_water_box_at_the_default_parameters(precision):
    """every Drude particle on its oxygen; padding, posq, velm and posDelta untouched (added_by); two calls add twice"""
    ctx, f = pme_context("P3", precision)
    assert f.num_terms == (1080, 2160, 0)
    added, e, _ = check_state("P3", precision, ctx, f)
    assert e[2:4] == (0.0, 0.0) and e[4] > 0 and e[7] != 0
    assert np.array_equal(added_by(ctx, f), added) and np.any(added != 0)
    ctx.close()


def test_p4_the_reciprocal_part_alone():
    """4 200 ions, no pair inside the cutoff, no exception: the buffer's change is the mesh force; pure-radix lines 16, 27, 25; a slot
    without a charge receives nothing"""
    ctx, f = pme_context("P4", "mixed")
    assert ctx.n == 4200 and f.pme[1] == (16, 27, 25)
    added, e, ref = check_state("P4", "mixed", ctx, f)
    assert e[0] == 0 and e[3] == 0 and e[7] == 0 and e[4] > 0
    q = pme_states()["P4", "mixed"][1][3][:, 0]
    assert np.array_equal(added[q == 0], np.zeros(((q == 0).sum(), 3), np.int64)) and (q == 0).sum() == 600
    assert np.all(np.abs(added.astype(L) / L(FIXED) - ref["recip"]) <= force_gate(ref))
    ctx.close()


@pytest.mark.parametrize("grid", THIN_GRIDS + MIXED_GRIDS)
def test_the_transform_alone(grid):
    """Q is exact, so phi checks the five transform launches and the influence function: the longest lines of every radix mix"""
    x, table, box, alpha = phi_state()
    ctx, f = context("double", rock_salt()[0], table, box, x=x)
    f.set_pme(alpha, *grid)
    f.compute()
    Q, phi = f.pme_grids()
    want_q, want_phi, scale = phi_checked(grid, L)
    assert Q.shape == grid[::-1] and np.array_equal(Q, want_q)
    off = np.abs(phi.astype(L) - want_phi)
    print(f"grid {grid}: phi off the reference by at most {float((off / scale).max()):.2e} of Phi_abs, the gate allows {GATE_PME:.1e}")
    assert np.all(off <= L(GATE_PME) * scale) and np.abs(want_phi).max() > 1e-3
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_properties(precision):
    s, _, info = system_b()
    table, pme = charged_b(), pme_states()["P2", precision][3]
    ctx, f = pme_context("P2", precision)
    full = added_by(ctx, f)
    Q, phi = f.pme_grids()
    assert np.array_equal(added_by(ctx, f), full) and np.any(full != 0)                          # the same bits twice
    Q2, phi2 = f.pme_grids()
    assert np.array_equal(Q, Q2) and np.array_equal(bits(phi), bits(phi2))
    # recorded into a graph and replayed
    torch = ctx.torch
    torch.cuda.synchronize(ctx.dev)
    f0 = snapshot(ctx)["force"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f.compute()
    torch.cuda.synchronize(ctx.dev)
    assert np.array_equal(snapshot(ctx)["force"], f0)            # recording runs nothing
    g.replay()
    torch.cuda.synchronize(ctx.dev)
    assert np.array_equal(planes(snapshot(ctx)["force"] - f0, ctx), full)
    del g
    # all charges 0: the reaction-field call's bits
    par = table[3].copy()
    par[:, 0] = 0
    f = NonbondedForces(ctx, table[:3] + (par,) + table[4:])
    plain = added_by(ctx, f)
    f.set_pme(*pme)
    assert np.array_equal(added_by(ctx, f), plain) and np.any(plain != 0)
    assert not np.any(f.pme_grids()[0])
    # tgnh_set_nonbonded_force drops the setting: the reaction-field twin's bits again
    plain_table = system_b()[1]
    f = NonbondedForces(ctx, plain_table, pme=pme)
    assert f.pme is not None
    f = NonbondedForces(ctx, plain_table)
    assert f.pme is None
    assert np.array_equal(added_by(ctx, f), twin("B", precision))
    f.set_pme(*pme)
    f.clear_pme()
    assert np.array_equal(added_by(ctx, f), twin("B", precision))
    ctx.close()
    # other handles over the same slots: the same integers, the same grids and the same energy bits
    got = []
    for mode, flags in (("TGNH", 0), ("TGNH", FLAG_GATHER), ("dualNH", 0)):
        ctx, f = pme_context("P2", precision, mode, flags)
        assert ctx.step_path()[0] == ("gather" if flags else "tiled")
        added = added_by(ctx, f, energy=True)
        e1, e2 = f.energy() + f.ewald_energy(), f.energy() + f.ewald_energy()
        assert bits(np.array(e1)).tolist() == bits(np.array(e2)).tolist()
        got.append((added, e1, f.pme_grids()))
        ctx.close()
    assert np.array_equal(got[0][0], full) and np.array_equal(got[0][2][0], Q) and np.array_equal(bits(got[0][2][1]), bits(phi))
    for added, e, (q_, phi_) in got[1:]:
        assert np.array_equal(added, full) and bits(np.array(e)).tolist() == bits(np.array(got[0][1])).tolist()
        assert np.array_equal(q_, Q) and np.array_equal(bits(phi_), bits(phi))
    # reversed molecules: the same charge grid, the same phi bits, the permuted force bits of the whole call
    s2, table2, perm = reversed_molecules(s, table)
    ctx, f = context(precision, s2, table2, BOX_B)
    f.set_pme(*pme)
    permuted = added_by(ctx, f)
    q_, phi_ = f.pme_grids()
    assert np.array_equal(q_, Q) and np.array_equal(bits(phi_), bits(phi)) and np.array_equal(permuted, full[perm])
    ctx.close()


def test_the_box_changes_between_two_calls():
    """G, V and the N / L of the force are formed on the device from the box of the call: no reset in between"""
    ctx, f = pme_context("P2", "mixed")
    check_state("P2", "mixed", ctx, f)
    set_box(ctx, BOX_B_MORE)
    check_state("P2 more", "mixed", ctx, f)
    ctx.close()


def test_sequencing_launch_counts_and_state_errors():
    s, _, info = system_b()
    table, pme = charged_b(), pme_states()["P2", "mixed"][3]
    ctx, f = context("mixed", s, table, BOX_B)
    lib, stream = ctx.lib, ctx._stream()
    ctx.timing(True)

    def launches(force):
        before = ctx.timing_read(_lib.KID_OTHER)[1]
        force.compute()
        return ctx.timing_read(_lib.KID_OTHER)[1] - before

    assert launches(f) == 6
    with pytest.raises(TgnhError, match="particle-mesh Ewald is off") as e:
        f.pme_grids()
    assert e.value.status == _lib.ERR_STATE
    f.set_ewald(*ewald_b())
    with pytest.raises(TgnhError, match="particle-mesh Ewald is off"):
        f.pme_grids()
    f.compute(energy=True)
    assert len(f.ewald_energy()) == 4
    f.set_pme(*pme)                                              # replaces the explicit sum: every query waits for a call
    for call in (f.energy, f.ewald_energy):
        with pytest.raises(TgnhError, match="want_energy") as e:
            call()
        assert e.value.status == _lib.ERR_STATE
    with pytest.raises(TgnhError, match="no tgnh_compute_nonbonded_force since") as e:
        f.pme_grids()
    assert e.value.status == _lib.ERR_STATE
    assert launches(f) == 14                                     # 6, the exclusion correction, spread, five transform launches, gather
    assert f.pme_grids()[0].shape == GRID_P2[::-1]
    with pytest.raises(TgnhError, match="want_energy"):          # a launch without want_energy is not one
        f.ewald_energy()
    f.compute(energy=True)
    first = f.ewald_energy()
    assert first == f.ewald_energy() and first[0] > 0
    assert lib.tgnh_get_pme_grids(ctx.h, stream, None, None) == _lib.TGNH_OK
    none = table[:4] + (table[4][:0], table[5][:0])              # no exception at all
    f = NonbondedForces(ctx, none, pme=pme)
    assert launches(f) == 12                                     # 5 + 0 + 7
    f.set_ewald(pme[0], 0, 0, 0)
    assert launches(f) == 5 and f.pme is None                    # the explicit sum with M = 0, as before
    ctx.timing(False)
    # inside a capture that has recorded this handle's call, the setter is refused and changes nothing
    f = NonbondedForces(ctx, table, pme=pme)
    f.compute()
    torch = ctx.torch
    torch.cuda.synchronize(ctx.dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f.compute()
        rc = lib.tgnh_set_nonbonded_pme(ctx.h, C.byref(pdesc()))
        message = lib.tgnh_last_error().decode()
        rc_clear = lib.tgnh_set_nonbonded_pme(ctx.h, None)
    assert rc == _lib.ERR_STATE and "outside the capture" in message and rc_clear == _lib.ERR_STATE
    assert f.pme == (pme[0], tuple(pme[1:]))
    f.set_pme(3.0, 10, 12, 15)                                   # ... and is taken again once the capture has ended
    assert f.pme == (3.0, (10, 12, 15)) and ctx.check() == 0
    ctx.close()
