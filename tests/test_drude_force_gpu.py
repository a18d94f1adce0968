"""GPU tests of the library's own DrudeForce (csrc/tgnh_drude_force.hip; tgnh_compute_drude_force, tgnh_get_drude_energy,
HipContext.drude_force).  The table, the states, the fp80 reference, its fp64 twin and the gate are those of
tests/test_drude_force.py, which checks the reference against finite differences of its own energy and measures the gate on the CPU.

Tolerances.
 * a slot that receives isotropic shares only: none.  Its entries change by the twin's rint(c 2^32), summed as integers.
 * every other entry: per contribution, GATE (16 x the margin between twin and reference, 8.3e-14) x the largest share component of
   that term x 2^32, plus one unit of fixed point (positions are read, not stored: single precision has no store to round).
 * independent of any reference: every term's shares add up to zero, so the buffer's total changes by 0 within half a unit per
   conversion, per plane.
 * the energies: GATE x the sum of |term energies|.
 * 20 steps against the oracle: tests/test_gpu_parity.py's gate as its docstring states it -- TOL in the precisions that carry fp64
   velocities; a float4 state "cannot hold 1e-6 against a double-precision oracle with a stiff Drude spring" and is bounded there by
   test_single_precision_deviation's figure, 2e-3 on velocities.  Here the bound is worked out for this system and never wider than
   that: 20 kicks of a Drude particle, each off by dt K3 2^-23 max|x| / m_D (the spring on two coordinates stored to half an ulp),
   over the largest velocity: 2.8e-4 (measured: 5.5e-5).  Positions are held to TOL in single too.
 * the Drude-only minimisation on the library's springs alone: the minimiser gates the root mean square of 3 x 64 force components at
   `tolerance`, so no component exceeds sqrt(192) x tolerance, and no Drude is further than that over k3 from its parent."""
import numpy as np
import pytest

from openmm_drudenose_amd import _lib
from openmm_drudenose_amd.drudetgnhplugin import HipContext, PREC_MIXED, TgnhError, FLAG_GATHER
from openmm_drudenose_amd.forces import DrudeForce
from openmm_drudenose_amd.system import DrudeSystem
from helpers import make_oracle, rel_err
from test_drude_force import PRECISIONS, GATE, FIXED, ONE_4PI_EPS0, L, drude_system, state, results, energies, integrator
from test_gpu_parity import TOL, integ

pytestmark = pytest.mark.gpu
_cache = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def context(precision, mode="TGNH", flags=0, table=True):
    """A context over the table's system with the state's arrays stored as they are; every w, velm, posDelta and the whole force
    buffer, padding included, carry patterns of their own."""
    s, tables = drude_system()
    st = state(precision)
    ctx = HipContext(s, integrator(), mode=mode, precision=precision, flags=flags)
    assert ctx.num_drude_force_terms == (67, len(tables[2])) and not ctx.drude_force             # the system's table went to the handle
    if not table:
        ctx.set_drude_force(None)
    t, n = ctx.torch, s.num_particles
    w = np.arange(n, dtype=np.float64)
    rng = np.random.default_rng(5)
    ctx.posq[:, :3] = t.tensor(st["posq"]).to(ctx.dev)
    ctx.posq[:, 3] = t.from_numpy(0.25 + w).to(ctx.dev, ctx.rdt)                                  # (charges come from the table, never from here)
    if ctx.precision == PREC_MIXED:
        ctx.posq_corr[:, :3] = t.tensor(st["corr"]).to(ctx.dev)
        ctx.posq_corr[:, 3] = t.from_numpy((0.5 + w).astype(np.float32)).to(ctx.dev)
    ctx.pos_delta[:] = t.from_numpy(rng.normal(size=(n, 4))).to(ctx.dev, ctx.mdt)
    ctx.velm[:, :3] = t.from_numpy(rng.normal(size=(n, 3))).to(ctx.dev, ctx.mdt)
    ctx.force[:] = t.from_numpy(rng.integers(-2 ** 40, 2 ** 40, 3 * ctx.padded)).to(ctx.dev)
    return ctx, s


def snapshot(ctx):
    return {k: (None if a is None else a.cpu().numpy().copy())
            for k, a in (("posq", ctx.posq), ("corr", ctx.posq_corr), ("delta", ctx.pos_delta), ("velm", ctx.velm), ("force", ctx.force))}


def same(a, b, keys):
    for k in keys:
        if a[k] is not None:
            assert np.array_equal(bits(a[k]), bits(b[k])), k


def planes(buf, ctx):
    return buf.reshape(3, ctx.padded)[:, :ctx.n].T.copy()


def expected(precision):
    """-> (exact [n, 3] int64: the isotropic springs' rint sums per slot, from the twin; near [n, 3] fp80: every other term's shares
    x 2^32 from the reference, unrounded; tol [n, 3]: what the gate allows; count [n]: conversions per slot)"""
    if ("expected", precision) not in _cache:
        n = drude_system()[0].num_particles
        exact, near, tol, count = np.zeros((n, 3), np.int64), np.zeros((n, 3), L), np.zeros((n, 3), L), np.zeros(n, np.int64)
        for (name, slots, rs, _, _), (_, _, ts, _, _) in zip(results(precision, L), results(precision, np.float64)):
            scale = np.max([np.abs(v).max(1) for v in rs], axis=0)[:, None]
            for s, r, t in zip(slots, rs, ts):
                np.add.at(count, s, 1)
                if name == "isotropic":
                    np.add.at(exact, s, np.rint(t * FIXED).astype(np.int64))
                else:
                    np.add.at(near, s, r * L(FIXED))
                    np.add.at(tol, s, np.broadcast_to(L(GATE) * scale * L(FIXED) + 1, r.shape))
        _cache["expected", precision] = (exact, near, tol, count)
    return _cache["expected", precision]


@pytest.mark.parametrize("precision", PRECISIONS)
def test_forces(precision):
    ctx, s = context(precision)
    n = s.num_particles
    before = snapshot(ctx)
    ctx.compute_drude_force()
    assert ctx.check() == 0
    after = snapshot(ctx)
    same(after, before, ("posq", "corr", "delta", "velm"))
    f0, f1 = planes(before["force"], ctx), planes(after["force"], ctx)
    added = f1 - f0
    exact, near, tol, count = expected(precision)
    pure = (count > 0) & (tol[:, 0] == 0)
    gated = tol[:, 0] > 0
    assert pure.sum() >= 20 and gated.any() and ((exact != 0).any(1) & gated).any() and count.max() >= 6
    assert np.array_equal(added[pure], exact[pure])                                             # isotropic shares only: the twin's integers
    miss = np.abs((added - exact).astype(L) - near)
    print(f"forces {precision}: largest miss {float(miss[gated].max()):.2f} units of fixed point, {float((miss[gated] / tol[gated]).max()):.2e} of what the gate "
          f"allows; up to {count.max()} conversions a slot, largest entry {np.abs(added).max() / FIXED:.1f} kJ/mol/nm")
    assert np.all(miss <= tol)
    # independent of any reference: every term's shares add up to zero
    total = added.sum(0)
    print(f"forces {precision}: the buffer's total changed by {list(total)} units ({count.sum()} conversions)")
    assert np.abs(total).max() <= 0.5 * count.sum()
    # slots in no term, the padding
    assert (count == 0).sum() >= 15 and np.array_equal(added[count == 0], np.zeros_like(added[count == 0]))
    pad0, pad1 = before["force"].reshape(3, ctx.padded)[:, n:], after["force"].reshape(3, ctx.padded)[:, n:]
    assert pad0.size > 0 and np.array_equal(pad0, pad1)
    # a second call adds the same integers again
    ctx.compute_drude_force()
    f2 = planes(snapshot(ctx)["force"], ctx)
    assert np.array_equal(f2 - f1, added)
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_energy_and_other_handles(precision):
    """The energies against the reference; asked twice, the same bits; the launch with want_energy adds the integers the plain one
    adds; a TGNH_FLAG_GATHER handle and a DUALNH handle over the same slots give the same integers and the same energy bits."""
    ref = results(precision, L)
    want = energies(ref)
    room = [L(GATE) * sum(np.abs(e).sum() for _, _, _, e, scr in ref if scr == which) for which in (False, True)]
    got = []
    for mode, flags in (("TGNH", 0), ("TGNH", FLAG_GATHER), ("dualNH", 0)):
        ctx, s = context(precision, mode, flags)
        assert ctx.step_path()[0] == ("gather" if flags else "tiled")
        f0 = snapshot(ctx)["force"]
        ctx.compute_drude_force(energy=True)
        e1, e2 = ctx.drude_energy(), ctx.drude_energy()
        assert ctx.check() == 0
        assert bits(np.array(e1)).tolist() == bits(np.array(e2)).tolist()
        got.append((snapshot(ctx)["force"] - f0, e1))
        ctx.close()
    e = got[0][1]
    print(f"energies {precision}: springs {e[0]:.6f} screened pairs {e[1]:.6f} kJ/mol; off the reference by {float(abs(L(e[0]) - want[0])):.2e} and "
          f"{float(abs(L(e[1]) - want[1])):.2e}, the gate allows {float(room[0]):.2e} and {float(room[1]):.2e}")
    assert abs(L(e[0]) - want[0]) <= room[0] and abs(L(e[1]) - want[1]) <= room[1] and e[0] > 0 and e[1] != 0
    for added, other in got[1:]:
        assert np.array_equal(added, got[0][0]) and bits(np.array(other)).tolist() == bits(np.array(e)).tolist()
    ctx, s = context(precision)                                                                 # the plain launch: the same integers
    f0 = snapshot(ctx)["force"]
    ctx.compute_drude_force()
    assert np.array_equal(snapshot(ctx)["force"] - f0, got[0][0])
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_state_and_empty_cases(precision):
    ctx, s = context(precision, table=False)
    assert ctx.num_drude_force_terms == (0, 0)
    before = snapshot(ctx)
    ctx.compute_drude_force()                                    # an empty table: TGNH_OK and nothing happens
    ctx.compute_drude_force(energy=True)
    same(snapshot(ctx), before, ("posq", "corr", "delta", "velm", "force"))
    with pytest.raises(TgnhError) as e:
        ctx.drude_energy()
    assert e.value.status == _lib.ERR_STATE
    ctx.set_drude_force(s.drude_force)
    ctx.compute_drude_force()                                    # a launch without want_energy is not one either
    with pytest.raises(TgnhError, match="want_energy") as e:
        ctx.drude_energy()
    assert e.value.status == _lib.ERR_STATE
    assert ctx.lib.tgnh_compute_drude_force(ctx.h, None, 0, ctx._stream()) == _lib.ERR_STATE
    ctx.compute_drude_force(energy=True)
    first = ctx.drude_energy()
    ctx.set_drude_force(s.drude_force)                           # a new table: its energy has not been computed
    with pytest.raises(TgnhError, match="want_energy"):
        ctx.drude_energy()
    ctx.compute_drude_force(energy=True)
    assert ctx.drude_energy() == first and ctx.check() == 0
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_captured(precision):
    """The call recorded into a graph on the context's stream and replayed once adds the integers the eager call added."""
    ctx, s = context(precision)
    torch = ctx.torch
    f0 = snapshot(ctx)["force"]
    ctx.compute_drude_force()
    torch.cuda.synchronize(ctx.dev)
    f1 = snapshot(ctx)["force"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.compute_drude_force()
    torch.cuda.synchronize(ctx.dev)
    assert np.array_equal(snapshot(ctx)["force"], f1)            # recording runs nothing
    g.replay()
    torch.cuda.synchronize(ctx.dev)
    assert np.array_equal(snapshot(ctx)["force"] - f1, f1 - f0) and np.any(f1 != f0)
    assert ctx.check() == 0
    # a want_energy launch that was only recorded has not run: it does not open the query; an eager one does
    ctx.set_drude_force(s.drude_force)                           # (a new table: g's buffers are gone, it is not replayed again)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        ctx.compute_drude_force(energy=True)
    with pytest.raises(TgnhError, match="want_energy") as e:
        ctx.drude_energy()
    assert e.value.status == _lib.ERR_STATE
    ctx.compute_drude_force(energy=True)
    eager = ctx.drude_energy()
    g2.replay()
    torch.cuda.synchronize(ctx.dev)
    assert ctx.drude_energy() == eager and eager[0] > 0 and ctx.check() == 0      # the replayed launch left the same rows
    ctx.close()


# ---------------------------------------------------------------------------
# isotropic systems: more than one work-group, the minimiser, the step
# ---------------------------------------------------------------------------
Q_D, ALPHA = -1.71636, 0.00097825
K3 = ONE_4PI_EPS0 * Q_D * Q_D / (ALPHA * (3.0 - 1.0 - 1.0))


def isotropic_system(pairs, lone, seed, spread=0.01):
    """`pairs` two-slot molecules (parent, Drude) with one isotropic row each and `lone` atoms, on a 0.4 nm lattice about the origin;
    Drude particles `spread` nm (normal, per component) off their parents; thermal velocities"""
    rng = np.random.default_rng(seed)
    n = 2 * pairs + lone
    side = int(np.ceil((pairs + lone) ** (1.0 / 3.0) - 1e-9))
    idx = np.arange(pairs + lone)
    centres = (np.stack([idx // (side * side), (idx // side) % side, idx % side], 1) - (side - 1) / 2.0) * 0.4
    pos, mass, resid = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int32)
    parent = 2 * np.arange(pairs)
    pos[parent], pos[parent + 1] = centres[:pairs], centres[:pairs] + rng.normal(0.0, spread, (pairs, 3))
    mass[parent], mass[parent + 1] = 15.9994 - 0.4, 0.4
    resid[parent], resid[parent + 1] = np.arange(pairs), np.arange(pairs)
    pos[2 * pairs:], mass[2 * pairs:], resid[2 * pairs:] = centres[pairs:], 22.99, pairs + np.arange(lone)
    vel = rng.normal(size=(n, 3)) * np.sqrt(0.0083144626 * 300.0 / mass)[:, None]
    vel[parent + 1] = vel[parent] + rng.normal(size=(pairs, 3)) * np.sqrt(0.0083144626 * 1.0 / 0.4)
    s = DrudeSystem(mass=mass, pair_drude=(parent + 1).astype(np.int32), pair_parent=parent.astype(np.int32), resid=resid, positions=pos,
                    velocities=vel, name=f"{pairs} isotropic pairs, {lone} lone atoms")
    f = DrudeForce()
    for p in parent:
        f.addParticle(p + 1, p, -1, -1, -1, Q_D, ALPHA)
    s.set_drude_force(f)
    return s


def spring_forces(s, x):
    """the isotropic springs restated in numpy: three lines"""
    t = K3 * (x[s.pair_drude] - x[s.pair_parent])
    f = np.zeros_like(x)
    f[s.pair_drude], f[s.pair_parent] = -t, t
    return f


@pytest.mark.parametrize("precision", PRECISIONS)
def test_more_than_one_work_group(precision):
    """700 isotropic pairs: 1400 receiving slots, six work-groups and six rows of energy.  The twin's integers, and the energy within
    GATE of the fp80 sum."""
    s = isotropic_system(700, 3, 11)
    ctx = HipContext(s, integrator(), mode="TGNH", precision=precision)
    ctx.force.zero_()
    ctx.compute_drude_force(energy=True)
    springs, screened = ctx.drude_energy()
    x = ctx.getPositions()
    got = planes(snapshot(ctx)["force"], ctx)
    assert np.array_equal(got, np.rint(spring_forces(s, x) * FIXED).astype(np.int64))
    d = (x[s.pair_drude] - x[s.pair_parent]).astype(L)
    want = (L(0.5) * L(K3) * (d * d).sum(1)).sum()
    print(f"700 pairs {precision}: springs {springs:.6f} kJ/mol, off the fp80 sum by {float(abs(L(springs) - want) / want):.2e} of it")
    assert abs(L(springs) - want) <= L(GATE) * want and screened == 0.0 and ctx.check() == 0
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_drude_particles_relax_in_a_uniform_field(precision):
    """64 isotropic pairs and five lone atoms in a uniform field E: force_fn puts q E on every Drude slot, the library's stage adds the
    springs, minimizeEnergy(drude_only=True) relaxes the Drude particles.  They start ON their parents and the field lies along
    (1, 1, 1), so every component of every pair's residual is the same number and the root mean square the minimiser gates IS the
    largest component: every Drude ends at q E / k3 from its parent within tolerance / k3.  Without the stage nothing pulls them
    back and the minimiser never converges."""
    s = isotropic_system(64, 5, 3, spread=0.0)
    ctx = HipContext(s, integrator(), mode="TGNH", precision=precision)
    torch = ctx.torch
    q = np.zeros(s.num_particles)
    q[s.pair_drude] = Q_D
    ctx.setCharges(q)
    E = np.array([-1400.0, -1400.0, -1400.0])                    # kJ/mol/nm/e: q E / k3 = 0.0057 nm per component
    drude = torch.from_numpy(np.asarray(s.pair_drude, np.int64)).to(ctx.dev)
    qE = torch.from_numpy(np.rint(Q_D * E * FIXED).astype(np.int64)).to(ctx.dev)

    def field(c):
        c.force.zero_()
        c.force.view(3, c.padded)[:, drude] += qE[:, None]
    ctx.force_fn = field
    ctx.drude_force = True
    tolerance = 1.0
    st = ctx.minimizeEnergy(tolerance=tolerance, maxIterations=20000, drude_only=True)
    assert ctx.check() == 0
    x = ctx.getPositions()
    d = x[s.pair_drude] - x[s.pair_parent]
    miss = np.abs(d - Q_D * E / K3).max()
    print(f"relaxation in a field, {precision}: converged {st.converged} after {st.iterations} iterations, rms force {st.rms_force:.3e}; "
          f"displacement {d[0]} nm, off q E / k3 by {miss:.2e} nm (allowed {tolerance / K3:.2e})")
    assert st.converged == 1 and st.moving == 64
    assert miss <= tolerance / K3
    assert np.abs(x[s.pair_parent] - s.positions[s.pair_parent]).max() <= 1e-7                 # the parents stayed (stored in the position type)
    stats = ctx.drude_statistics()
    stored_q = ctx.posq[:, 3].to(torch.float64).cpu().numpy()[s.pair_drude]
    want = (stored_q[:, None] * d).sum(0)
    print(f"relaxation in a field, {precision}: induced dipole {stats.induced_dipole} e nm")
    assert np.abs(stats.induced_dipole - want).max() <= 1e-13 * np.abs(stored_q[:, None] * d).sum() and np.abs(want).min() > 0.5
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_minimise_on_the_library_springs_without_a_force_fn(precision):
    """drude_force = True and no force_fn: the call-out is the harness force -- switched off here, k_drude = k_tether = 0 -- plus the
    library's stage, so the minimiser must take the loop that runs compute_forces().  The Drude particles start 0.01 nm off and end on
    their parents; the loop that knows the harness force alone would see no force at all and leave them where they are."""
    s = isotropic_system(64, 5, 5, spread=0.01)
    ctx = HipContext(s, integrator(), mode="TGNH", precision=precision, k_drude=0.0, k_tether=0.0)
    assert ctx.force_fn is None
    ctx.drude_force = True
    tolerance = 1.0
    st = ctx.minimizeEnergy(tolerance=tolerance, maxIterations=20000, drude_only=True)
    assert ctx.check() == 0
    x = ctx.getPositions()
    d0 = np.abs(s.positions[s.pair_drude] - s.positions[s.pair_parent]).max()
    d = np.abs(x[s.pair_drude] - x[s.pair_parent]).max()
    allowed = np.sqrt(3 * 64) * tolerance / K3
    print(f"minimiser on the library's springs alone, {precision}: converged {st.converged} after {st.iterations} iterations, rms force "
          f"{st.rms_force:.3e}; largest Drude displacement {d0:.2e} -> {d:.2e} nm (allowed {allowed:.2e})")
    assert st.converged == 1 and st.moving == 64 and st.iterations > 0
    assert d0 > 0.01 and d <= allowed
    assert np.abs(ctx.getForces()).max() <= np.sqrt(3 * 64) * tolerance * (1 + 1e-6)      # the buffer is the call-out's at the final positions
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_steps_against_the_oracle(precision):
    """20 steps of HipContext.step with a force_fn that zeroes the buffer and drude_force = True, against the oracle stepped with the
    springs restated in numpy: the stage stands where the force call-out stands."""
    s = isotropic_system(64, 5, 7, spread=0.004)
    it = integ(chains=2, dt=0.0005)
    ctx = HipContext(s, it, mode="TGNH", precision=precision)
    ctx.force_fn = lambda c: c.force.zero_()
    ctx.drude_force = True
    ctx.compute_forces()
    o = make_oracle(s, ctx.group, ctx.num_groups, "TGNH", it)
    pos, vel = ctx.getPositions(), s.velocities.copy()           # (the positions as the context stores them)
    f = spring_forces(s, pos)
    for _ in range(20):
        o.step_begin(pos, vel, f)
        f = spring_forces(s, pos)
        o.step_end(vel, f)
    ctx.step(20)
    assert ctx.check() == 0 and ctx.time()[1] == 20
    ep, ev = rel_err(ctx.getPositions(), pos), rel_err(ctx.getVelocities(), vel)
    print(f"20 steps on the library's springs, {precision}: pos {ep:.2e} vel {ev:.2e}")
    vel_gate = TOL
    if precision == "single":
        # a stored coordinate is off by up to half an ulp, 2^-24 |x|, and the spring sees the difference of two: a force off by up to
        # K3 2^-23 max|x|, a kick of the Drude particle (0.4 u) off by dt times that over its mass -- every step the same way at worst
        vel_gate = 20 * it.getStepSize() * K3 * 2.0 ** -23 * np.abs(pos).max() / 0.4 / np.abs(vel).max()
        print(f"20 steps on the library's springs, single: the velocities' gate {vel_gate:.2e}")
        assert TOL < vel_gate <= 2e-3                            # (never wider than test_single_precision_deviation's figure)
    assert ep <= TOL and ev <= vel_gate
    assert np.abs(pos - s.positions).max() > 1e-4                # it moved
    ctx.close()
