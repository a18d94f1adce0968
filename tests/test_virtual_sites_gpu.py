"""GPU tests of the library's virtual-site stage (csrc/tgnh_virtual_sites.hip; tgnh_compute_virtual_sites,
tgnh_distribute_virtual_site_forces, HipContext(library_sites=True), site_forces, minimizeEnergy with sites).  The table, the
states, the fp80 reference, its fp64 twin and the gate are those of tests/test_virtual_sites.py, which checks the reference against
finite differences and measures the gate on the CPU.

Tolerances (the measure: per site, the largest difference over its components -- its coordinates, or its three shares -- over the
largest of them by magnitude in the reference).
 * the two average kinds: no tolerance.  The stored coordinates are the twin's, rounded as the store rounds (mixed: fp32 value and
   fp32 residual; single: once), bit for bit; the fixed-point sums are the twin's rint(c 2^32), as integers.
 * out of plane, local coordinates, double and mixed: GATE = 16 x the margin between twin and reference (1.4e-13).  Mixed precision
   stores 48 bits of a coordinate (3.6e-15): inside it.
 * single precision, placement: 2^-22.  The arithmetic is the same fp64 one on the fp32 positions; its result is rounded once to
   fp32 (2^-24 of the component) at a value that may sit across a rounding boundary from the reference's: the reason
   tests/test_constraints_gpu.py gives for the same figure.
 * distribution, every precision: an entry that receives from such a site is within GATE x that site's largest share component
   x 2^32, plus one unit of fixed point, per contribution (positions are read, not stored: single precision has no store to round).
 * independent of any reference: the buffer's total changes by the sum of the sites' forces, within half a unit per contribution."""
import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import HipContext, PREC_MIXED, TgnhError
from openmm_drudenose_amd.system import DrudeSystem
from helpers import make_oracle, rel_err
from test_virtual_sites import (TWO, THREE, PLANE, LOCAL, PRECISIONS, GATE, FIXED, TIP5, PLANE_W, site_system, state, results, evaluate,
                                integrator)
from test_gpu_parity import CONSTRAINED, TOL, integ, bind_groups

pytestmark = pytest.mark.gpu

SINGLE_GATE = 2.0 ** -22
L = np.longdouble


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def context(precision):
    """A context over the table's system with the state's arrays stored as they are; every w, velm, posDelta and the padding of the
    force buffer carry patterns of their own."""
    s, kinds, atoms, params = site_system()
    st = state(precision)
    ctx = HipContext(s, integrator(), mode="TGNH", precision=precision)
    assert ctx.num_virtual_sites == 0 and not ctx.constrained
    ctx.set_virtual_sites(kinds, atoms, params)
    assert ctx.num_virtual_sites == len(kinds) and ctx.constrained
    t, n = ctx.torch, s.num_particles
    w = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(5)
    ctx.posq[:, :3] = t.tensor(st["posq"]).to(ctx.dev)
    ctx.posq[:, 3] = t.from_numpy(0.25 + w).to(ctx.dev, ctx.rdt)
    if ctx.precision == PREC_MIXED:
        ctx.posq_corr[:, :3] = t.tensor(st["corr"]).to(ctx.dev)
        ctx.posq_corr[:, 3] = t.from_numpy((0.5 + w).astype(np.float32)).to(ctx.dev)
    ctx.pos_delta[:] = t.from_numpy(rng.normal(size=(n, 4))).to(ctx.dev, ctx.mdt)
    ctx.velm[:, :3] = t.from_numpy(rng.normal(size=(n, 3))).to(ctx.dev, ctx.mdt)
    ctx.force[:] = t.from_numpy(rng.integers(-2 ** 40, 2 ** 40, 3 * ctx.padded))                 # (the padding keeps these)
    ctx.force.view(3, ctx.padded)[:, :n] = t.from_numpy(np.ascontiguousarray(st["force"].T))
    return ctx, s, st


def snapshot(ctx):
    return {k: (None if a is None else a.cpu().numpy().copy())
            for k, a in (("posq", ctx.posq), ("corr", ctx.posq_corr), ("delta", ctx.pos_delta), ("velm", ctx.velm), ("force", ctx.force))}


def same(a, b, keys, rows=None):
    for k in keys:
        if a[k] is not None:
            x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
            assert np.array_equal(bits(x), bits(y)), k


@pytest.mark.parametrize("precision", PRECISIONS)
def test_placement(precision):
    ctx, s, st = context(precision)
    _, kinds, atoms, params = site_system()
    before = snapshot(ctx)
    ctx.compute_virtual_sites()
    assert ctx.check() == 0
    after = snapshot(ctx)
    site = atoms[:, 0]
    twin, ref = results(precision, np.float64)[0], results(precision, L)[0]
    avg = (kinds == TWO) | (kinds == THREE)
    # the averages: the twin's bits
    if precision == "double":
        assert np.array_equal(bits(after["posq"][site[avg], :3]), bits(twin[avg]))
    else:
        hi = twin.astype(np.float32)
        assert np.array_equal(bits(after["posq"][site[avg], :3]), bits(hi[avg]))
        if precision == "mixed":
            assert np.array_equal(bits(after["corr"][site[avg], :3]), bits((twin - hi.astype(np.float64)).astype(np.float32)[avg]))
    # the other kinds: the gate
    got = after["posq"][site, :3].astype(L) + (after["corr"][site, :3].astype(L) if precision == "mixed" else 0)
    err = np.abs(got - ref).max(1) / np.abs(ref).max(1)
    gate = SINGLE_GATE if precision == "single" else GATE
    print(f"placement {precision}: out of plane {float(err[kinds == PLANE].max()):.2e} local coordinates {float(err[kinds == LOCAL].max()):.2e} "
          f"averages {float(err[avg].max()):.2e} of the site's largest coordinate (gate {gate:.1e})")
    assert err.max() <= gate
    # nothing else is written
    other = np.setdiff1d(np.arange(s.num_particles), site)
    same(after, before, ("posq", "corr"), other)
    assert np.array_equal(bits(after["posq"][:, 3]), bits(before["posq"][:, 3]))
    if precision == "mixed":
        assert np.array_equal(bits(after["corr"][:, 3]), bits(before["corr"][:, 3]))
    same(after, before, ("delta", "velm", "force"))
    assert not np.any(np.all(after["posq"][site, :3] == before["posq"][site, :3], axis=1))      # every site moved (the state has them 3 pm off)
    ctx.compute_virtual_sites()                                                                 # the parents have not moved: the same bits again
    same(snapshot(ctx), after, ("posq", "corr"))
    ctx.close()


def expected_distribution(precision, padded):
    """-> (exact [n, 3] int64: the averages' rint sums per receiving slot; near [n, 3] fp80: the other kinds' shares x 2^32 from the
    reference, unrounded; tol [n, 3]: what the gate allows; count [n]: contributions per slot)"""
    s, kinds, atoms, params = site_system()
    n = s.num_particles
    twin, ref = results(precision, np.float64)[1], results(precision, L)[1]
    exact, near, tol, count = np.zeros((n, 3), np.int64), np.zeros((n, 3), L), np.zeros((n, 3), L), np.zeros(n, np.int64)
    for k in range(len(kinds)):
        for r in range(2 if kinds[k] == TWO else 3):
            p = atoms[k, 1 + r]
            count[p] += 1
            if kinds[k] in (TWO, THREE):
                exact[p] += np.rint(twin[k, r] * FIXED).astype(np.int64)
            else:
                near[p] += ref[k, r] * L(FIXED)
                tol[p] += L(GATE) * np.abs(ref[k]).max() * L(FIXED) + 1
    return exact, near, tol, count


def planes(buf, ctx):
    return buf.reshape(3, ctx.padded)[:, :ctx.n].T.copy()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_distribution(precision):
    ctx, s, st = context(precision)
    _, kinds, atoms, params = site_system()
    n = s.num_particles
    before = snapshot(ctx)
    ctx.distribute_site_forces()
    assert ctx.check() == 0
    after = snapshot(ctx)
    same(after, before, ("posq", "corr", "delta", "velm"))
    f0, f1 = planes(before["force"], ctx), planes(after["force"], ctx)
    assert np.array_equal(f0, st["force"])
    added = f1 - f0
    exact, near, tol, count = expected_distribution(precision, ctx.padded)
    pure = (count > 0) & (tol[:, 0] == 0)
    assert pure.any() and (tol[:, 0] > 0).any() and ((exact != 0).any(1) & (tol[:, 0] > 0)).any()       # average-only slots, gated ones, and slots with both
    assert np.array_equal(added[pure], exact[pure])                                             # the averages: the twin's integers
    miss = np.abs((added - exact).astype(L) - near)
    gated = tol[:, 0] > 0
    print(f"distribution {precision}: largest miss {float(miss[gated].max()):.2f} units of fixed point, of {float((miss[gated] / tol[gated]).max()):.2e} of what the gate allows; "
          f"up to {count.max()} contributions a slot")
    assert np.all(miss <= tol)
    # independent of any reference: what the parents received is what the sites held
    total, held = added.sum(0), f0[atoms[:, 0]].sum(0)
    print(f"distribution {precision}: total received - total held = {list(total - held)} units ({count.sum()} contributions)")
    assert np.abs(total - held).max() <= 0.5 * count.sum()
    # the sites' own entries, every slot that receives nothing, the padding
    assert np.array_equal(added[count == 0], np.zeros_like(added[count == 0])) and count[atoms[:, 0]].max() == 0 and count[n - 1] > 0
    pad0, pad1 = before["force"].reshape(3, ctx.padded)[:, n:], after["force"].reshape(3, ctx.padded)[:, n:]
    assert pad0.size > 0 and np.array_equal(pad0, pad1)
    # a second call adds the same integers again
    ctx.distribute_site_forces()
    f2 = planes(snapshot(ctx)["force"], ctx)
    assert np.array_equal(f2 - f1, added)
    ctx.close()
    # two runs give identical buffers
    ctx2 = context(precision)[0]
    ctx2.distribute_site_forces()
    assert np.array_equal(snapshot(ctx2)["force"], after["force"])
    ctx2.close()


def test_the_launching_calls_without_a_table_or_a_buffer():
    s = site_system()[0]
    ctx = HipContext(s, integrator(), mode="TGNH", precision="mixed")
    before = snapshot(ctx)
    ctx.compute_virtual_sites()                                  # an empty table: TGNH_OK and nothing happens
    ctx.distribute_site_forces()
    same(snapshot(ctx), before, ("posq", "corr", "delta", "velm", "force"))
    assert ctx.lib.tgnh_distribute_virtual_site_forces(ctx.h, None, ctx._stream()) == _lib.ERR_STATE
    ctx.close()


# ---------------------------------------------------------------------------
# the whole path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["mixed", "double"])
@pytest.mark.parametrize("mode", ["dualNH", "TGNH"])
def test_constrained_path_parity_with_library_sites(mode, precision):
    """test_constrained_path_parity's recipe and gate (tests/test_gpu_parity.py) with library_sites=True: rigid SWM4 water, its M
    sites in the library's table, 20 steps of the split step against the oracle's constrained loop."""
    s, g, ng = CONSTRAINED["rigid SWM4 water (3 constraints + M virtual site per molecule)"]()
    it = integ(chains=2, hardwall=0.02)
    it.setConstraintTolerance(1e-10)
    if mode == "TGNH":
        bind_groups(it, g, ng)
    else:
        g, ng = np.zeros_like(g), 1
    ctx = HipContext(s, it, mode=mode, precision=precision, library_sites=True)
    assert ctx.constrained and not ctx._harness_sites and ctx.num_virtual_sites == s.num_particles // 5 == len(s.site_atoms)
    o = make_oracle(s, g, ng, mode, it)
    pos, vel, x0 = s.positions.copy(), s.velocities.copy(), ctx.sites()
    f = o.harness_force(pos, x0, synth.K_DRUDE, synth.K_TETHER)
    o.run_harness_constrained(pos, vel, f, x0, synth.K_DRUDE, synth.K_TETHER, 1e-10, 20)
    ctx.step(20)
    assert ctx.check() == 0
    gp, gv = ctx.getPositions(), ctx.getVelocities()
    ep, ev = rel_err(gp, pos), rel_err(gv, vel)
    print(f"constrained, library sites, {mode} {precision}: pos {ep:.2e} vel {ev:.2e}")
    assert ep <= TOL and ev <= TOL
    sa, w = s.site_atoms, s.site_weights
    expect = (w[:, [0]] * gp[sa[:, 1]] + w[:, [1]] * gp[sa[:, 2]]) + w[:, [2]] * gp[sa[:, 3]]
    assert np.array_equal(gp[sa[:, 0]], expect) if precision == "double" else np.abs(gp[sa[:, 0]] - expect).max() <= 2.0 ** -48 * np.abs(expect).max()
    ctx.close()


def test_step_loops_place_the_library_sites():
    """The C loop, the force_fn branch of step() and a replayed capture issue the same launches in the same order: the same bits."""
    out = []
    for how in ("c", "python", "graph"):
        s, g, ng = synth.water_box(64, rigid=True)
        it = integ(chains=1, hardwall=0.02, dt=0.0005)
        bind_groups(it, g, ng)
        ctx = HipContext(s, it, mode="TGNH", precision="mixed", library_sites=True)
        if how == "python":
            ctx.force_fn = lambda c: _lib.load().tgnh_harness_force(c.h, c._x0_arg(), c.k_drude, c.k_tether, c.force.data_ptr(), c._stream())
        ctx.step(2)
        if how == "graph":
            replay = ctx.capture_steps(3)
            for _ in range(2):
                replay()
        else:
            ctx.step(6)
        assert ctx.time()[1] == 8 and ctx.check() == 0
        out.append((ctx.getPositions(), ctx.getVelocities()))
        ctx.close()
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0]) and np.array_equal(out[0][1], other[1])
    m = out[0][0].reshape(-1, 5, 3)                              # O, D, H1, H2, M
    assert np.abs(m[:, 4] - ((0.786646558 * m[:, 0] + 0.106676721 * m[:, 2]) + 0.106676721 * m[:, 3])).max() <= 1e-14


# ---------------------------------------------------------------------------
# the minimiser
# ---------------------------------------------------------------------------
def five_site_waters(n_mol=27, spacing=0.31):
    """unconstrained five-site waters on a lattice: O, H1, H2 and two out-of-plane lone pairs, no Drude particle"""
    side = int(np.ceil(n_mol ** (1.0 / 3.0) - 1e-9))
    idx = np.arange(n_mol)
    centres = np.stack([idx // (side * side), (idx // side) % side, idx % side], 1) * spacing + 0.2
    pos = (centres[:, None, :] + TIP5[None]).reshape(-1, 3)
    base = 5 * idx
    kinds = np.full(2 * n_mol, PLANE, np.int32)
    atoms = np.concatenate([np.stack([base + 3, base, base + 1, base + 2], 1), np.stack([base + 4, base, base + 1, base + 2], 1)])
    params = np.zeros((2 * n_mol, 12))
    params[:n_mol, :3] = PLANE_W
    params[n_mol:, :3] = (PLANE_W[0], PLANE_W[1], -PLANE_W[2])
    pos[atoms[:, 0]] = evaluate(kinds, atoms, params, pos, np.zeros_like(pos), np.float64)[0]
    s = DrudeSystem(mass=np.tile([15.9994, 1.008, 1.008, 0.0, 0.0], n_mol), pair_drude=np.zeros(0, np.int32), pair_parent=np.zeros(0, np.int32),
                    resid=np.repeat(idx, 5).astype(np.int32), positions=pos, velocities=np.zeros_like(pos), name=f"tip5-{n_mol}")
    s.set_site_table(kinds, atoms, params)
    return s


K_TETHER = 1.0e4                 # kJ/mol/nm^2


@pytest.mark.parametrize("precision", PRECISIONS)
def test_minimise_with_forces_on_sites(precision):
    """A harmonic tether on EVERY slot, the massless sites included, to points 0.02 nm off: the sites' forces reach the minimiser
    only through distribute_site_forces.  Every massive slot moves; FIRE converges, the energy the test computes itself has dropped,
    and every site sits on its placement."""
    s = five_site_waters()
    ctx = HipContext(s, integrator(), mode="TGNH", precision=precision, library_sites=True)
    assert ctx.num_virtual_sites == 54 and ctx.constrained and not ctx._has_clusters
    torch = ctx.torch
    target = s.positions + np.random.default_rng(31).normal(0.0, 0.02, s.positions.shape)
    x0 = torch.from_numpy(target).to(ctx.dev)

    def tether(c):
        x = c.posq[:, :3].to(torch.float64)
        if c.posq_corr is not None:
            x = x + c.posq_corr[:, :3].to(torch.float64)
        c.force.view(3, c.padded)[:, :c.n] = torch.round(-K_TETHER * (x - x0) * FIXED).to(torch.int64).t()

    def energy():
        d = ctx.getPositions() - target
        return 0.5 * K_TETHER * float((d * d).sum())
    ctx.force_fn = tether
    ctx.site_forces = True
    ctx.compute_virtual_sites()
    e0 = energy()
    st = ctx.minimizeEnergy(tolerance=1.0, maxIterations=5000)
    assert ctx.check() == 0
    e1 = energy()
    print(f"minimiser with site forces, {precision}: converged {st.converged} after {st.iterations} iterations, rms force {st.rms_force:.3f}, energy {e0:.3f} -> {e1:.3f} kJ/mol")
    assert st.converged == 1 and st.moving == 3 * 27
    assert e1 < e0
    x = ctx.getPositions()
    want = evaluate(s.site_table_kinds, s.site_table_atoms, s.site_table_params, x, np.zeros_like(x), L)[0]
    got = x[s.site_table_atoms[:, 0]]
    err = float((np.abs(got - want).max(1) / np.abs(want).max(1)).max())
    assert err <= (SINGLE_GATE if precision == "single" else GATE)
    assert np.abs(x[s.mass > 0] - s.positions[s.mass > 0]).max() > 1e-3                         # the massive slots moved
    ctx.close()
    # without site_forces the sites' forces are lost: the same call ends at another, higher, energy
    ctx = HipContext(s, integrator(), mode="TGNH", precision=precision, library_sites=True)
    ctx.force_fn = tether
    st2 = ctx.minimizeEnergy(tolerance=1.0, maxIterations=5000)
    assert st2.converged == 1 and energy() > e1
    ctx.close()


def test_minimise_is_still_refused_with_constraints_or_harness_sites():
    s = synth.water_box(8, rigid=True)[0]
    for kw in ({}, {"library_sites": True}):                     # harness sites and clusters; library sites, but clusters
        ctx = HipContext(s, integrator(), mode="TGNH", precision="mixed", **kw)
        with pytest.raises(TgnhError, match="constraints or virtual sites") as e:
            ctx.minimizeEnergy()
        assert e.value.status == _lib.ERR_STATE
        ctx.close()
