"""GPU tests of the direct constraint solver (tgnh_constraints.hip; tgnh_apply_constraints, tgnh_apply_velocity_constraints,
HipContext(direct_constraints=True)) against the oracle's converged SHAKE.  The states, the shapes and the reference are those of
tests/test_constraints.py, which also checks that the reference converged.

Tolerances.  The measure is, per cluster, the largest difference between the device's result and the oracle's over the cluster's
atoms and components, over the largest component (by magnitude) of the oracle's result in that cluster -- the corrected
displacements, or velocities, themselves: what a store rounds.
 * double, mixed: 1e-10.  Two independent fp64 solutions of the same equations -- Newton on the multipliers and SHAKE at 1e-14, the
   one linear solve and the iterative velocity stage at 1e-12 -- agreed to 3.0e-12 and 3.8e-13 on the CPU; 1e-10
   leaves about 30 x over that for another order of operations.  Both store posDelta and velm in fp64.
 * single: 2^-22.  The solve is the same fp64 one; its result is rounded once to fp32 (2^-24 of the component, at most 2^-24 of the
   measure's denominator), taken at a value that may sit across a rounding boundary from the oracle's: a factor 2, and 2 over.
 * independent of any reference (double, mixed): |d'^2 - d^2| <= 1e-12 d^2 with the new positions x + delta' formed in fp64 (their
   rounding at |x| < 8 nm, 8.9e-16 nm, is 2e-14 of a squared 0.1 nm bond), and |r . dv| / r^2 <= 1e-12 sqrt(w_i + w_j).
Measured figures: profiles/constraints.md."""
import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import HipContext, PREC_MIXED
from openmm_drudenose_amd.system import DrudeSystem
from helpers import make_oracle, rel_err
from test_constraints import (SHAPES, PRECISIONS, shape, state, reference, integrator, constraints_of, rate_violation)
from test_gpu_parity import CONSTRAINED, TOL, integ, bind_groups

pytestmark = pytest.mark.gpu

GATE = {"double": 1e-10, "mixed": 1e-10, "single": 2.0 ** -22}
APPLY_TOL = 1e-10            # the gate handed to the apply calls: four Newton iterations leave these states at fp64 rounding


def context(name, precision, direct=True):
    """A context over a shape with the state's arrays stored as they are; w of every array carries a pattern of its own."""
    s = shape(name)[0]
    st = state(name, precision)
    ctx = HipContext(s, integrator(), mode="TGNH", precision=precision, direct_constraints=direct)
    t, n = ctx.torch, s.num_particles
    w = np.arange(n, dtype=np.float64)
    ctx.posq[:, :3] = t.tensor(st["posq"]).to(ctx.dev)
    ctx.posq[:, 3] = t.from_numpy(0.25 + w).to(ctx.dev, ctx.rdt)
    if ctx.precision == PREC_MIXED:
        ctx.posq_corr[:, :3] = t.tensor(st["corr"]).to(ctx.dev)
        ctx.posq_corr[:, 3] = t.from_numpy((0.5 + w).astype(np.float32)).to(ctx.dev)
    ctx.pos_delta[:, :3] = t.tensor(st["delta"]).to(ctx.dev)
    ctx.pos_delta[:, 3] = t.from_numpy(0.75 + w).to(ctx.dev, ctx.mdt)
    ctx.velm[:, :3] = t.tensor(st["vel"]).to(ctx.dev)
    return ctx, s, st


def snapshot(ctx):
    return {k: (None if a is None else a.cpu().numpy().copy()) for k, a in (("posq", ctx.posq), ("corr", ctx.posq_corr), ("delta", ctx.pos_delta), ("velm", ctx.velm))}


def cluster_error(s, got, ref):
    """the measure of the module docstring -> its largest value over the clusters"""
    worst = 0.0
    for at in s.cluster_atoms:
        at = at[at >= 0]
        worst = max(worst, float(np.abs(got[at] - ref[at]).max() / np.abs(ref[at]).max()))
    return worst


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_one_application_against_converged_shake(name, precision):
    ctx, s, st = context(name, precision)
    k = len(s.cluster_atoms)
    assert ctx.constraint_clusters == (k, 0) and ctx.constrained
    before = snapshot(ctx)
    ctx.apply_constraints(APPLY_TOL)
    ctx.apply_velocity_constraints(APPLY_TOL)
    assert ctx.check() == 0                                             # a fresh context whose tolerances hold
    after = snapshot(ctx)
    ref_d, ref_v = reference(name, precision)
    got_d, got_v = after["delta"][:, :3].astype(np.float64), after["velm"][:, :3].astype(np.float64)
    ed, ev = cluster_error(s, got_d, ref_d), cluster_error(s, got_v, ref_v)
    i, j, d, _ = constraints_of(s)
    xn = st["x"] + got_d                                                # x + delta' formed in fp64
    bonds = float((np.abs(((xn[i] - xn[j]) ** 2).sum(1) - d * d) / (d * d)).max())
    rates = rate_violation(s, st["x"], got_v)
    print(f"direct solver {name} {precision}: positions {ed:.2e} velocities {ev:.2e} of the cluster's largest component (gate {GATE[precision]:.1e}); "
          f"bonds {bonds:.2e} rates {rates:.2e}")
    assert ed <= GATE[precision] and ev <= GATE[precision]
    if precision != "single":
        assert bonds <= 1e-12 and rates <= 1e-12
    # untouched data, bit for bit: slots in no cluster (Drude particles, M sites, anions), every w, posq and posq_correction
    inside = np.zeros(s.num_particles, bool)
    inside[s.cluster_atoms[s.cluster_atoms >= 0]] = True
    assert (~inside).any() or name == "xh3"
    for key in ("delta", "velm"):
        assert np.array_equal(after[key][~inside], before[key][~inside]), key
        assert np.array_equal(after[key][:, 3], before[key][:, 3]), key
        assert not np.array_equal(after[key][inside, :3], before[key][inside, :3]), key
    assert np.array_equal(after["posq"], before["posq"])
    if before["corr"] is not None:
        assert np.array_equal(after["corr"], before["corr"])
    ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_constraint_without_a_solution_sets_status_bit_1(precision):
    """One X-H cluster whose displacement makes the new bond vector perpendicular to the old one, with twice its length: no multiplier
    satisfies |s + lambda c r| = d (|s| > d and s . r = 0), and the Jacobian 2 (s . r) c is zero.  Every number below is exact in
    fp32, so the zero is a zero on the device.  The kernel divides by it and stores what comes out: a flagged non-solution, not a
    device fault."""
    s = DrudeSystem(mass=np.array([12.0, 1.0]), pair_drude=np.zeros(0, np.int32), pair_parent=np.zeros(0, np.int32), resid=np.zeros(2, np.int32),
                    positions=np.array([[3.0, -2.75, 0.5], [3.125, -2.75, 0.5]]), velocities=np.zeros((2, 3)), name="x-h")
    s.set_clusters([[0, 1, -1, -1]], [[0.125, 0, 0, 0, 0, 0]])
    ctx = HipContext(s, integrator(), mode="TGNH", precision=precision, direct_constraints=True)
    assert ctx.constraint_clusters == (1, 0) and ctx.check() == 0
    ctx.pos_delta[:, :3] = ctx.torch.tensor([[0.125, 0.25, 0.0], [0.0, 0.0, 0.0]], dtype=ctx.mdt, device=ctx.dev)      # s = (0, 0.25, 0), r = (-0.125, 0, 0)
    ctx.apply_constraints(1e-5)
    assert ctx.status_flags() == 2                                      # bit 1 and no other
    assert ctx.check() == 2                                             # ... which is no failure: the handle goes on answering
    assert ctx.num_constraint_clusters() == 1 and ctx.time()[1] == 0 and ctx.num_thermostats() == 3
    assert np.array_equal(ctx.posq.cpu().numpy()[:, :3], s.positions)
    ctx.close()


@pytest.mark.parametrize("precision", ["mixed", "double"])
@pytest.mark.parametrize("mode", ["dualNH", "TGNH"])
@pytest.mark.parametrize("name", list(CONSTRAINED))
def test_constrained_path_parity_with_the_direct_solver(name, mode, precision):
    """test_constrained_path_parity's recipe (tests/test_gpu_parity.py) with direct_constraints=True: the split step with the direct
    solver in the constraint call-outs' places against the oracle's constrained loop, whose SHAKE runs at 1e-10."""
    s, g, ng = CONSTRAINED[name]()
    it = integ(chains=2, hardwall=0.02)
    it.setConstraintTolerance(1e-10)
    if mode == "TGNH":
        bind_groups(it, g, ng)
    else:
        g, ng = np.zeros_like(g), 1
    ctx = HipContext(s, it, mode=mode, precision=precision, direct_constraints=True)
    assert ctx.constrained and ctx.constraint_clusters == (len(s.cluster_atoms), 0)
    o = make_oracle(s, g, ng, mode, it)
    pos, vel, x0 = s.positions.copy(), s.velocities.copy(), ctx.sites()
    f = o.harness_force(pos, x0, synth.K_DRUDE, synth.K_TETHER)
    o.run_harness_constrained(pos, vel, f, x0, synth.K_DRUDE, synth.K_TETHER, 1e-10, 50)
    ctx.step(50)
    assert ctx.check() == 0
    gp, gv = ctx.getPositions(), ctx.getVelocities()
    ep, ev = rel_err(gp, pos), rel_err(gv, vel)
    print(f"constrained, direct solver, {name} {mode} {precision}: pos {ep:.2e} vel {ev:.2e}")
    assert ep <= TOL and ev <= TOL
    a, d = s.cluster_atoms, s.cluster_dist
    for k, (i, j) in enumerate(s.PAIRS):
        m = d[:, k] > 0
        if m.any():
            r = np.linalg.norm(gp[a[m, i]] - gp[a[m, j]], axis=1)
            assert np.abs(r - d[m, k]).max() <= 1e-7 * d[m, k].max()
    if s.site_atoms is not None:
        sa, w = s.site_atoms, s.site_weights
        expect = sum(w[:, [m]] * gp[sa[:, m + 1]] for m in range(3))
        assert np.abs(gp[sa[:, 0]] - expect).max() <= 1e-7
    ctx.close()


def test_python_step_loop_runs_the_direct_stages():
    """The force_fn branch of step() against the C loop: the same launches in the same order, so the same bits."""
    out = []
    for own_force in (False, True):
        s, g, ng = synth.water_box(27, rigid=True)
        it = integ(chains=1, hardwall=0.02, dt=0.0005)
        bind_groups(it, g, ng)
        ctx = HipContext(s, it, mode="TGNH", precision="mixed", direct_constraints=True)
        if own_force:
            ctx.force_fn = lambda c: _lib.load().tgnh_harness_force(c.h, c._x0_arg(), c.k_drude, c.k_tether, c.force.data_ptr(), c._stream())
        ctx.step(6)
        assert ctx.check() == 0
        out.append((ctx.getPositions(), ctx.getVelocities()))
        ctx.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    pos = out[1][0].reshape(-1, 5, 3)
    assert np.allclose(np.linalg.norm(pos[:, 2] - pos[:, 0], axis=1), 0.09572, rtol=2e-5)


def test_graph_replay_with_the_direct_solver_matches_eager():
    """test_graph_replay_of_the_constrained_step_matches_eager's assertion (tests/test_gpu_parity.py) for the new launches."""
    out = []
    for graphed in (False, True):
        s, g, ng = synth.water_box(216, rigid=True)
        it = integ(chains=1, hardwall=0.02, dt=0.0005)
        bind_groups(it, g, ng)
        ctx = HipContext(s, it, mode="TGNH", precision="double", direct_constraints=True)
        assert ctx.constraint_clusters == (216, 0)
        ctx.step(3)
        if graphed:
            replay = ctx.capture_steps(5)
            for _ in range(4):
                replay()
        else:
            ctx.step(20)
        assert ctx.time()[1] == 23 and ctx.check() == 0
        out.append((ctx.getPositions(), ctx.getVelocities(), ctx.thermostat_state(1)))
        ctx.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)
    pos = out[1][0].reshape(-1, 5, 3)                         # O, D, H1, H2, M
    assert np.allclose(np.linalg.norm(pos[:, 2] - pos[:, 0], axis=1), 0.09572, rtol=2e-5)
    assert np.allclose(np.linalg.norm(pos[:, 3] - pos[:, 2], axis=1), 0.15139, rtol=2e-5)


def test_the_default_leaves_everything_with_the_harness():
    out = []
    for kw in ({}, {"direct_constraints": False}):
        s, g, ng = synth.water_box(64, rigid=True)
        it = integ(chains=1, hardwall=0.02, dt=0.0005)
        bind_groups(it, g, ng)
        ctx = HipContext(s, it, mode="TGNH", precision="mixed", **kw)
        assert ctx.constraint_clusters == (0, 64)
        ctx.step(10)
        assert ctx.check() == 0
        out.append((ctx.getPositions(), ctx.getVelocities()))
        ctx.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_velocity_draw_projects_with_the_direct_solver():
    """setVelocitiesToTemperature runs the new velocity stage next to the harness': the drawn velocities satisfy the constraints."""
    s, g, ng = synth.water_box(64, rigid=True)
    it = integ(chains=1)
    bind_groups(it, g, ng)
    ctx = HipContext(s, it, mode="TGNH", precision="double", direct_constraints=True)
    ctx.setVelocitiesToTemperature(300.0, randomSeed=7)
    assert ctx.check() == 0
    assert rate_violation(s, ctx.getPositions(), ctx.getVelocities()) <= 1e-12
    ctx.close()
