"""GPU tests of Ewald summation on the library's NonbondedForce (csrc/tgnh_ewald.hip, tgnh_nonbonded.hip's Ewald instantiation;
tgnh_set_nonbonded_ewald, tgnh_get_ewald_energy, forces.NonbondedForces).  The states, the fp80 reference, its fp64 twin and the gate
are those of tests/test_ewald.py, which holds the reference to the Madelung energy, to its independence of alpha and to finite
differences of its own energy, and measures the gate on the CPU.

Tolerances.
 * forces, per slot and component: GATE_EWALD (16 x the margin between twin and reference) x S_i, the sum of the absolute values of
   the terms the slot receives, plus 2^-33 per converted contribution of the slot (force_gate).  The device's erfc, erf, exp and
   sincospi are not numpy's, so no bit-for-bit twin exists with Ewald on.
 * the eight energies: GATE_EWALD x the sum of the terms' magnitudes, each; the rock-salt total: the same over all eight.
 * exact, with no reference: kmax (0, 0, 0) leaves the direct and exclusion parts alone, whose integer shares cancel and permute with
   the slots; with all charges 0 the Ewald call adds the reaction-field call's bits; after tgnh_set_nonbonded_force the call is
   tests/test_nonbonded.py's twin again, bit for bit; twice, from another handle, replayed from a graph: the same bits."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import _lib
from openmm_drudenose_amd.drudetgnhplugin import TgnhError, FLAG_GATHER
from openmm_drudenose_amd.forces import NonbondedForces
from test_nonbonded import PRECISIONS, FIXED, K, L, BOX_B, BOX_B_MORE, system_a, system_b
from test_nonbonded_gpu import context, added_by, set_box, load, twin, reversed_molecules
from test_bonded_forces_gpu import bits, snapshot, planes
from test_ewald import (GATE_EWALD, ENERGIES, MADELUNG, ROCK_A, ewald_states, evaluated, force_gate, rock_salt, lattice_e4, kvectors,
                        charged_b, ewald_b, desc)

pytestmark = pytest.mark.gpu
SYSTEMS = {"E1": lambda: rock_salt()[0], "E2": lambda: system_b()[0], "E3": lambda: system_a()[0], "E4": lambda: lattice_e4()[0]}


def ewald_context(name, precision, mode="TGNH", flags=0):
    """a context over the state's system with Ewald on -> (ctx, the NonbondedForces on it)"""
    x, table, box, ewald = ewald_states()[name, precision]
    ctx, f = context(precision, SYSTEMS[name[:2]](), table, box, mode, flags, x=x)
    f.set_ewald(*ewald)
    assert f.ewald == (ewald[0], tuple(ewald[1:]), len(kvectors(ewald[1:])))
    return ctx, f


def check_forces(name, precision, added):
    ref = evaluated(name, precision, L)
    off = np.abs(added.astype(L) / L(FIXED) - ref["force"])
    gate = force_gate(ref)
    worst = float((off / np.maximum(gate, L(1e-300))).max())
    print(f"{name} {precision}: forces off the reference by at most {worst:.3f} of the gate; largest force {float(np.abs(ref['force']).max()):.1f} kJ/mol/nm, "
          f"largest deviation {float(off.max()):.2e}")
    assert np.all(off <= gate)
    return ref


def check_energies(name, precision, f):
    ref = evaluated(name, precision, L)
    e = f.energy() + f.ewald_energy()
    for m, kind in enumerate(ENERGIES):
        off, room = abs(L(e[m]) - ref["energy"][m]), L(GATE_EWALD) * ref["mag"][m]
        print(f"{name} {precision}: {kind} {e[m]:.6f} kJ/mol, off the reference by {float(off):.2e}, the gate allows {float(room):.2e}")
        assert off <= room
    return e, ref


@pytest.mark.parametrize("precision", PRECISIONS)
def test_e1_rock_salt(precision):
    """64 ions, M = 58 824 (920 tiles of vectors, the last one ragged): the Madelung energy, forces of zero, and a jittered state"""
    ctx, f = ewald_context("E1", precision)
    assert f.ewald[2] == 58824 and f.ewald[2] % 64 != 0
    added = added_by(ctx, f, energy=True)
    ref = check_forces("E1", precision, added)
    e, _ = check_energies("E1", precision, f)
    want = -L(32) * L(MADELUNG) * L(K) / L(ROCK_A / 2)
    total = sum(L(v) for v in e)
    print(f"rock salt {precision}: total {float(total):.9f} against the Madelung energy {float(want):.9f}")
    assert abs(total - want) <= L(GATE_EWALD) * ref["mag"].sum()
    if precision == "double":                                    # (the lattice as fp64 holds it; a float4 lattice is off it by 1e-8 nm)
        assert np.all(np.abs(added.astype(L) / L(FIXED)) <= force_gate(ref))
        x = ewald_states()["E1 jitter", "double"][0]
        load(ctx, x, precision)
        added = added_by(ctx, f, energy=True)
        ref = check_forces("E1 jitter", precision, added)
        check_energies("E1 jitter", precision, f)
        assert np.abs(ref["force"]).max() > 10
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_e2_system_b(precision):
    """exclusions, evaluated exceptions, molecules outside the box, three kmax on three edges; then a net charge"""
    ctx, f = ewald_context("E2", precision)
    assert len(set(f.ewald[1])) == 3 and ctx.padded > ctx.n
    added = added_by(ctx, f, energy=True)
    check_forces("E2", precision, added)
    e, _ = check_energies("E2", precision, f)
    assert all(v != 0 for m, v in enumerate(e) if m != 6)
    f = NonbondedForces(ctx, charged_b(), ewald=ewald_b())
    added = added_by(ctx, f, energy=True)
    check_forces("E2 charged", precision, added)
    e, ref = check_energies("E2 charged", precision, f)
    assert e[6] < -1e-3 and abs(charged_b()[3][:, 0].sum()) > 0.1
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_e3_system_a(precision):
    """the water box with every Drude particle on its oxygen (the exclusion correction's r2 == 0 branch) at the default tolerance's
    parameters; padding, posq, velm and posDelta untouched (added_by); two calls add twice"""
    ctx, f = ewald_context("E3", precision)
    assert f.num_terms == (1080, 2160, 0)
    added = added_by(ctx, f, energy=True)
    check_forces("E3", precision, added)
    e, _ = check_energies("E3", precision, f)
    assert e[2:4] == (0.0, 0.0) and e[7] != 0
    assert np.array_equal(added_by(ctx, f), added) and np.any(added != 0)
    ctx.close()


def test_e4_the_reciprocal_part_alone():
    """4 200 ions (a ragged second part of slots), no pair inside the cutoff, no exception: the buffer's change is the reciprocal
    force, M = 346; a slot without a charge receives nothing"""
    ctx, f = ewald_context("E4", "mixed")
    assert ctx.n == 4200 and f.ewald[2] == 346
    added = added_by(ctx, f, energy=True)
    ref = check_forces("E4", "mixed", added)
    e, _ = check_energies("E4", "mixed", f)
    assert e[0] == 0 and e[3] == 0 and e[7] == 0 and e[4] > 0
    q = ewald_states()["E4", "mixed"][1][3][:, 0]
    assert np.array_equal(added[q == 0], np.zeros(((q == 0).sum(), 3), np.int64)) and (q == 0).sum() == 600
    off = np.abs(added.astype(L) / L(FIXED) - ref["recip"])
    assert np.all(off <= force_gate(ref)) and np.all(ref["count"] == (q != 0))
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_exact_properties(precision):
    s, table, info = system_b()
    alpha = ewald_b()[0]
    ctx, f = context(precision, s, table, BOX_B)
    ctx.timing(True)
    # kmax (0, 0, 0): the direct and exclusion parts alone
    f.set_ewald(alpha, 0, 0, 0)
    before = ctx.timing_read(_lib.KID_OTHER)[1]
    direct = added_by(ctx, f)
    assert ctx.timing_read(_lib.KID_OTHER)[1] == before + 7      # cell, scan, place, rank, pairs, exceptions, exclusion correction
    assert np.array_equal(direct.sum(0), np.zeros(3, np.int64)) and np.any(direct != 0)
    assert not np.array_equal(direct, twin("B", precision))
    f.set_ewald(*ewald_b())
    before = ctx.timing_read(_lib.KID_OTHER)[1]
    full = added_by(ctx, f)
    assert ctx.timing_read(_lib.KID_OTHER)[1] == before + 10     # ... and sum, finalise, force: three more
    assert np.array_equal(added_by(ctx, f), full) and not np.array_equal(full, direct)           # the same bits twice
    ctx.timing(False)
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
    neutral = table[:3] + (par,) + table[4:]
    f = NonbondedForces(ctx, neutral)
    plain = added_by(ctx, f)
    f.set_ewald(*ewald_b())
    assert np.array_equal(added_by(ctx, f), plain) and np.any(plain != 0)
    # tgnh_set_nonbonded_force drops the setting: the twin's bits again
    f = NonbondedForces(ctx, table, ewald=ewald_b())
    assert f.ewald is not None
    f = NonbondedForces(ctx, table)
    assert f.ewald is None
    assert np.array_equal(added_by(ctx, f), twin("B", precision))
    f.set_ewald(*ewald_b())
    f.clear_ewald()
    assert np.array_equal(added_by(ctx, f), twin("B", precision))
    ctx.close()
    # other handles over the same slots: the same integers and the same energy bits
    got = []
    for mode, flags in (("TGNH", 0), ("TGNH", FLAG_GATHER), ("dualNH", 0)):
        ctx, f = ewald_context("E2", precision, mode, flags)
        assert ctx.step_path()[0] == ("gather" if flags else "tiled")
        added = added_by(ctx, f, energy=True)
        e1, e2 = f.energy() + f.ewald_energy(), f.energy() + f.ewald_energy()
        assert bits(np.array(e1)).tolist() == bits(np.array(e2)).tolist()
        got.append((added, e1))
        ctx.close()
    assert np.array_equal(got[0][0], full)
    for added, e in got[1:]:
        assert np.array_equal(added, got[0][0]) and bits(np.array(e)).tolist() == bits(np.array(got[0][1])).tolist()
    # reversed molecules with kmax (0, 0, 0): the permuted bits
    s2, table2, perm = reversed_molecules(s, table)
    ctx, f = context(precision, s2, table2, BOX_B)
    f.set_ewald(alpha, 0, 0, 0)
    assert np.array_equal(added_by(ctx, f), direct[perm])
    ctx.close()


def test_the_box_changes_between_two_calls():
    """A_m, k_m, E_bg and the prefactors are formed on the device from the box of the call: no reset in between"""
    ctx, f = ewald_context("E2", "mixed")
    check_forces("E2", "mixed", added_by(ctx, f, energy=True))
    set_box(ctx, BOX_B_MORE)
    added = added_by(ctx, f, energy=True)
    check_forces("E2 more", "mixed", added)
    check_energies("E2 more", "mixed", f)
    ctx.close()


def test_sequencing_launch_counts_and_state_errors():
    s, table, info = system_b()
    ewald = ewald_b()
    ctx, f = context("mixed", s, table, BOX_B)
    lib, stream = ctx.lib, ctx._stream()
    ctx.timing(True)

    def launches(force):
        before = ctx.timing_read(_lib.KID_OTHER)[1]
        force.compute()
        return ctx.timing_read(_lib.KID_OTHER)[1] - before

    assert launches(f) == 6
    with pytest.raises(TgnhError, match="Ewald summation is off") as e:
        f.ewald_energy()
    assert e.value.status == _lib.ERR_STATE
    f.compute(energy=True)
    assert len(f.energy()) == 4
    f.set_ewald(*ewald)                                          # slot 0 changes its meaning: both queries wait for a want_energy call
    for call in (f.energy, f.ewald_energy):
        with pytest.raises(TgnhError, match="want_energy") as e:
            call()
        assert e.value.status == _lib.ERR_STATE
    assert launches(f) == 10                                     # charged exceptions: 6 + 1 + 3
    with pytest.raises(TgnhError, match="want_energy"):          # a launch without want_energy is not one
        f.ewald_energy()
    f.compute(energy=True)
    first = f.ewald_energy()
    assert first == f.ewald_energy() and lib.tgnh_get_ewald_energy(ctx.h, stream, None) == _lib.ERR_ARG
    f.set_ewald(ewald[0], 0, 0, 0)
    assert launches(f) == 7                                      # M = 0: three fewer
    f.compute(energy=True)
    e = f.ewald_energy()
    assert e[0] == 0 and e[1:] == first[1:]
    none = table[:4] + (table[4][:0], table[5][:0])              # no exception at all
    f = NonbondedForces(ctx, none, ewald=ewald)
    assert launches(f) == 8                                      # 5 + 0 + 3
    par = table[3].copy()
    par[:, 0] = 0
    f = NonbondedForces(ctx, table[:3] + (par,) + table[4:], ewald=ewald)
    assert launches(f) == 9                                      # the evaluated exceptions' launch, no charged row: 6 + 0 + 3
    ctx.timing(False)
    # inside a capture that has recorded this handle's call, the setter is refused and changes nothing
    f = NonbondedForces(ctx, table, ewald=ewald)
    f.compute()
    torch = ctx.torch
    torch.cuda.synchronize(ctx.dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f.compute()
        rc = lib.tgnh_set_nonbonded_ewald(ctx.h, C.byref(desc()))
        message = lib.tgnh_last_error().decode()
        rc_clear = lib.tgnh_set_nonbonded_ewald(ctx.h, None)
    assert rc == _lib.ERR_STATE and "outside the capture" in message and rc_clear == _lib.ERR_STATE
    assert f.ewald == (ewald[0], tuple(ewald[1:]), len(kvectors(ewald[1:])))
    f.set_ewald(3.0, 3, 4, 5)                                    # ... and is taken again once the capture has ended
    assert f.ewald == (3.0, (3, 4, 5), 346) and ctx.check() == 0
    ctx.close()
