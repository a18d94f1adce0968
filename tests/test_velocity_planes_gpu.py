"""The one-launch step with its velocities in three planes (tgnh_vplanes.hip) against the same build kept on velm.

Between two flushes of a DEFER_SCALE | RESIDENT_STEP sequence wstep_kernel may keep the velocities in x | y | z planes of the
library's own and take 1/m from a per-pattern table; TGNH_VELOCITY_PLANES=0 in the environment at tgnh_create keeps a handle on
velm.  The two forms run the same arithmetic in the same order, so EVERY comparison here is bit for bit (np.array_equal):
positions, velocities after a flush, thermostat_state(0 / 1), last_kinetic_energies.  The reference of each comparison is the
same call sequence on a handle created with the switch off; the parity tests hold both forms against the oracle.

Single precision stays on velm whatever the switch says: there the planes kernel and the velm kernel, compiled apart, do not
give the same bits, and equal bits are what keeps the layout a private matter.  Its cases run all the same: they
hold that such a handle never goes live and is what it was.

Shapes: the smallest water boxes at which the tile bookkeeping can go wrong -- 7 molecules (one partial wave tile), 13 (a full
tile and one of a single molecule), 1001 (83 full tiles and a partial one: work-groups with and without a tile), 3000 (wavefronts
that walk several tiles forward and back where the device holds fewer wavefronts than tiles).

The hard wall: the synthetic boxes start their Drude particles 140 sigma inside the 0.02 nm wall most tests switch on, so here the
wall is switched on in the live handle, once the planes are live, at 1 / 1.3 of the largest Drude-parent distance the device
reports: the step that follows bounces at least that pair (with this step size a Drude particle moves 0.1 sigma of its spring per
step: the pair neither comes inside nor reaches twice the wall before the wall is applied).  That it did is asserted as tests/test_hardwall_gpu.py does: the same steps
from a handle that never has a wall end elsewhere.
"""
import contextlib
import os

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import (DrudeTGNHIntegrator, HipContext, TgnhError, FLAG_DEFER_SCALE, FLAG_RESIDENT_STEP,
                                                   FLAG_WAVE_TILES)

pytestmark = pytest.mark.gpu

FLAGS = FLAG_DEFER_SCALE | FLAG_RESIDENT_STEP | FLAG_WAVE_TILES
DT = 0.0001          # (a Drude particle moves 0.1 sigma of its spring per step, see above)
T = 8                # PLANES_AFTER_STEPS (tgnh_step.cpp), asserted against the library's answer in every run


@contextlib.contextmanager
def planes_switch(on):
    old = os.environ.get("TGNH_VELOCITY_PLANES")
    if on:
        os.environ.pop("TGNH_VELOCITY_PLANES", None)
    else:
        os.environ["TGNH_VELOCITY_PLANES"] = "0"
    try:
        yield
    finally:
        os.environ.pop("TGNH_VELOCITY_PLANES", None)
        if old is not None:
            os.environ["TGNH_VELOCITY_PLANES"] = old


_SYSTEMS = {}


def water(n):
    if n not in _SYSTEMS:
        _SYSTEMS[n] = synth.water_box(n)
    return _SYSTEMS[n]


def context(system, planes, mode="TGNH", precision="mixed", chains=1, wall=0.0, flags=FLAGS):
    s, g, ng = system
    it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, DT, 20, chains, True, True)
    it.setMaxDrudeDistance(wall)
    if mode == "TGNH":
        for _ in range(ng):
            it.addTempGroup()
        it._particleTempGroup = np.ascontiguousarray(g, np.int32)
    with planes_switch(planes):
        return HipContext(s, it, mode=mode, precision=precision, flags=flags)


def snapshot(ctx):
    """everything the comparisons are made of (the velocity read-back flushes: the planes are left)"""
    return [ctx.getPositions(), ctx.getVelocities(), ctx.thermostat_state(0), ctx.thermostat_state(1), ctx.last_kinetic_energies()]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def live(ctx):
    return ctx.velocity_planes()[0]


# ---------------------------------------------------------------------------------------------------------------------
# steady state: every shape, precision, chain length and mode; the taken hard wall; odd and even step counts
# ---------------------------------------------------------------------------------------------------------------------
def steady_run(n, mode, precision, chains, planes, with_wall=True):
    """-> (positions right after the first step with the wall, snapshots at an odd and at an even step count, the wall)"""
    ctx = context(water(n), planes, mode, precision, chains)
    planes = planes and precision != "single"                # (what the library answers and does; module docstring)
    try:
        assert ctx.resident_kernel() == "wstep_kernel"
        assert ctx.velocity_planes() == (False, planes, 0, T)
        ctx.step(T + 1)                                      # the first begin has nothing pending (the plain launches), then T one-launch steps
        assert ctx.velocity_planes() == (False, planes, T if planes else 0, T)
        ctx.step(1)                                          # ... and the next one runs on the planes
        assert ctx.velocity_planes() == (planes, planes, T + 1 if planes else 0, T) and bool(ctx.pending_state() & 0x400) == planes
        v = 12 if precision == "single" else 24              # V r, V r/w without the 1/m word
        expect = ctx.n * (3 * (v if planes else v * 4 // 3) + 2 * 24 + 2 * (16 if precision == "single" else 32))
        assert ctx.algorithmic_bytes(_lib.KID_STEP) == expect
        far = ctx.drude_statistics(threshold=0.0).max_distance          # (reads positions: nothing is settled)
        wall = far / 1.3
        assert live(ctx) == planes and wall > 0
        if with_wall:
            ctx.integrator.setMaxDrudeDistance(wall)
        ctx.step(1)
        assert live(ctx) == planes
        after_wall = ctx.getPositions()                      # (positions never lag)
        ctx.step(2)                                          # T + 5 steps: odd
        assert ctx.time()[1] == T + 5 and live(ctx) == planes
        odd = snapshot(ctx)
        assert not live(ctx)
        ctx.step(T + 3)                                      # the plain begin, T steps on velm, two on the planes: T + 5 + T + 3, even
        assert ctx.time()[1] == 2 * T + 8 and live(ctx) == planes
        even = snapshot(ctx)
        flags = ctx.check()
        assert flags & ~1 == 0 and (mode == "TGNH" or flags == 0), flags      # (bits 3 and 4 among them: no meeting timed out)
        return after_wall, odd, even, wall
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["TGNH", "dualNH"])
@pytest.mark.parametrize("chains", [1, 3])
@pytest.mark.parametrize("precision", ["single", "mixed", "double"])
@pytest.mark.parametrize("n", [7, 13, 1001, 3000])
def test_steps_on_the_planes_are_the_steps_on_velm(n, precision, chains, mode):
    on = steady_run(n, mode, precision, chains, True)
    off = steady_run(n, mode, precision, chains, False)
    assert on[3] == off[3]
    assert np.array_equal(on[0], off[0]), "positions differ after the first step with the wall"
    assert same(on[1], off[1]), "an odd number of steps"
    assert same(on[2], off[2]), "an even number of steps"
    # the wall's branch was taken, on the planes: the same steps without a wall end elsewhere
    free = steady_run(n, mode, precision, chains, True, with_wall=False)
    assert free[3] == on[3] and not np.array_equal(free[0], on[0])


# ---------------------------------------------------------------------------------------------------------------------
# transitions: 30 steps interleaved with whatever may come between them
# ---------------------------------------------------------------------------------------------------------------------
def midstep(ctx, fn):
    """between tgnh_step_begin and tgnh_step_end nothing is pending: the only place where a deferred handle lets velocities be set"""
    ctx.step_begin()
    ctx.compute_forces()
    fn(ctx)
    ctx.step_end()


def op_get_velocities(ctx):
    ctx.getVelocities()
    return False


def op_kinetic_energy(ctx):
    ctx.kinetic_energy()
    ctx.compute_kinetic_energies()
    return False


def op_set_velocities_after_flush(ctx):
    """between steps a deferred handle refuses (the next thermostat half has run): the refusal must leave both forms alike;
    inside a step it is taken"""
    v = ctx.getVelocities() * 0.999
    with pytest.raises(TgnhError) as e:
        ctx.setVelocities(v)
    assert e.value.status == _lib.ERR_STATE

    def put(c):
        c.flush()
        c.setVelocities(c.getVelocities() * 0.999)
    midstep(ctx, put)
    ctx.extra_steps = 1
    return False


def op_remove_cm(ctx):
    midstep(ctx, lambda c: c.removeCMMotion())
    ctx.extra_steps = 1
    return False


def op_rescale(ctx):
    midstep(ctx, lambda c: c.rescale_to_temperature(310.0, 1.0))
    ctx.extra_steps = 1
    return False


def op_draw(ctx):
    midstep(ctx, lambda c: c.setVelocitiesToTemperature(300.0, randomSeed=7))
    ctx.extra_steps = 1
    return False


def op_drude_statistics(ctx):
    ctx.drude_statistics(threshold=1e-4)
    return None                                              # a query of positions: the planes stay as they are


OPS = {"getVelocities": op_get_velocities, "kinetic-energy": op_kinetic_energy, "set_velocities": op_set_velocities_after_flush,
       "cm-removal": op_remove_cm, "rescale": op_rescale, "draw": op_draw, "drude-statistics": op_drude_statistics}


def transition_run(opname, planes, precision):
    ctx = context(water(1001), planes, precision=precision, wall=0.02)
    try:
        taken, seen = 0, []
        for _ in range(2):                                   # on an interval: twice in the 30 steps
            ctx.step(T + 3)
            taken += T + 3
            assert live(ctx) == planes                       # the hysteresis rule: more than T one-launch steps in a row since the last settle
            ctx.extra_steps = 0
            stays = OPS[opname](ctx)
            taken += ctx.extra_steps
            assert live(ctx) == (planes if stays is None else stays)
            seen.append(ctx.velocity_planes())
        ctx.step(30 - taken)
        assert ctx.time()[1] == 30
        seen.append(ctx.velocity_planes())
        out = snapshot(ctx)
        assert ctx.check() == 0
        return out, seen
    finally:
        ctx.close()


@pytest.mark.parametrize("precision", ["mixed", "double"])
@pytest.mark.parametrize("opname", list(OPS))
def test_thirty_steps_interleaved_with(opname, precision):
    on, seen_on = transition_run(opname, True, precision)
    off, seen_off = transition_run(opname, False, precision)
    assert same(on, off)
    assert all(s == (False, False, 0, T) for s in seen_off)
    print(opname, seen_on)
    # what the hysteresis rule predicts of the last stretch: a settle between two steps is followed by one plain begin and then
    # one-launch steps (8 steps: 7 of them), one inside a step by one-launch steps alone (6 steps), and a query of positions
    # settles nothing (29 one-launch steps behind the first plain begin, on the planes since the ninth)
    if opname == "drude-statistics":
        assert seen_on == [(True, True, T + 2, T), (True, True, 2 * T + 5, T), (True, True, 29, T)]
    else:
        assert seen_on == [(False, True, 0, T)] * 2 + [(False, True, 7 if opname in ("getVelocities", "kinetic-energy") else 6, T)]


def test_a_checkpoint_restored_into_a_fresh_handle():
    """positions, velocities, thermostat and clock taken after 14 steps (the planes live) and put into a fresh handle, 16 steps on"""
    def run(planes):
        a = context(water(1001), planes, wall=0.02)
        b = None
        try:
            a.step(14)
            assert live(a) == planes
            pos, vel, clock = a.getPositions(), a.getVelocities(), a.time()
            assert not live(a)
            thermo = [a.thermostat_state(w) for w in range(3)]
            b = context(water(1001), planes, wall=0.02)
            b.setPositions(pos); b.setVelocities(vel); b.compute_forces()
            for w, arr in enumerate(thermo):
                b.set_thermostat_state(w, arr)
            b.set_time(*clock)
            b.step(16)
            assert b.time()[1] == 30 and live(b) == planes
            a.step(16)
            return snapshot(a) + snapshot(b)
        finally:
            a.close()
            if b is not None:
                b.close()
    assert same(run(True), run(False))


@pytest.mark.parametrize("start", ["before", "after"])
def test_recorded_steps_replayed(start):
    """capture_steps(5) replayed four times.  Started after the planes have gone live the recording holds steps on the planes (bit 10
    of the pending state is part of what a recording is checked against); started before, the recording holds steps on velm, no
    conversion is baked into it, and the handle stays on velm afterwards: its graph may be replayed again at any time."""
    def run(planes):
        ctx = context(water(1001), planes, wall=0.02)
        try:
            ctx.step(T + 2 if start == "after" else 3)
            assert live(ctx) == (planes and start == "after")
            replay = ctx.capture_steps(5)
            for _ in range(4):
                replay()
            ctx.torch.cuda.synchronize()
            assert live(ctx) == (planes and start == "after")
            assert ctx.velocity_planes()[1] == (planes and start == "after")
            ctx.step(T + 2)
            assert live(ctx) == (planes and start == "after")
            return snapshot(ctx) + [np.array(ctx.time())]
        finally:
            ctx.close()
    assert same(run(True), run(False))


def test_a_recording_is_not_replayed_from_the_other_layout():
    """steps recorded on the planes, replayed, a velocity read-back (the planes are left), two eager steps (every other pending bit
    is what it was at the recording) and the replay again: its launches would read the planes as the read-back left them.  The
    replay refuses; recorded again from where the handle stands, the steps are those of a handle on velm."""
    def run(planes):
        ctx = context(water(1001), planes, wall=0.02)
        try:
            ctx.step(T + 2)
            replay = ctx.capture_steps(4)
            replay()
            ctx.torch.cuda.synchronize()
            ctx.getVelocities()
            ctx.step(2)
            assert not live(ctx)
            if planes:
                with pytest.raises(TgnhError) as e:
                    replay()
                assert e.value.status == _lib.ERR_STATE
                replay = ctx.capture_steps(4)                # (on velm: pins the handle there)
                assert ctx.velocity_planes()[1] is False
            replay()
            ctx.torch.cuda.synchronize()
            return snapshot(ctx) + [np.array(ctx.time())]
        finally:
            ctx.close()
    assert same(run(True), run(False))


# ---------------------------------------------------------------------------------------------------------------------
# handles that never go live
# ---------------------------------------------------------------------------------------------------------------------
def test_a_caller_that_flushes_every_step_never_converts():
    def run(planes):
        ctx = context(water(1001), planes, wall=0.02)
        try:
            for _ in range(30):
                ctx.step(1)
                assert not live(ctx)
                ctx.flush()
                assert ctx.velocity_planes() == (False, planes, 0, T)
            return snapshot(ctx)
        finally:
            ctx.close()
    assert same(run(True), run(False))


def test_a_caller_that_settles_every_t_steps_never_converts():
    """T steps between two queries are one plain begin and T - 1 one-launch steps: below the threshold"""
    ctx = context(water(13), True)
    try:
        for _ in range(3):
            ctx.step(T)
            assert ctx.velocity_planes() == (False, True, T - 1, T)
            ctx.last_kinetic_energies()
            assert ctx.velocity_planes() == (False, True, 0, T)
    finally:
        ctx.close()


def test_tiles_that_are_not_all_patterned_stay_on_velm():
    def run(planes):
        ctx = context(synth.mixed(60, 6), planes, wall=0.02)
        try:
            assert ctx.resident_kernel() == "wstep_kernel"   # (the one-launch step over wave tiles, but not a handle for the planes)
            assert ctx.velocity_planes() == (False, False, 0, T)
            ctx.step(T + 5)
            assert ctx.velocity_planes() == (False, False, 0, T)
            return snapshot(ctx)
        finally:
            ctx.close()
    assert same(run(True), run(False))


@pytest.mark.parametrize("precision", ["mixed", "double"])
def test_an_inverse_mass_that_is_not_the_table_s_keeps_the_handle_on_velm(precision):
    """one slot's w one unit in the last place off before the first step: the check of the first conversion finds it, the handle
    stays on velm for good, and the results are those of the handle that never tried"""
    def run(planes):
        ctx = context(water(1001), planes, precision=precision, wall=0.02)
        try:
            w = ctx.velm[2503, 3].item()
            assert w > 0
            ctx.velm[2503, 3] = float(np.nextafter(w, 2 * w))
            assert ctx.velm[2503, 3].item() != w
            ctx.step(T + 1)
            assert ctx.velocity_planes() == (False, planes, T if planes else 0, T)
            ctx.step(4)                                      # the conversion ran, found the slot, and was dropped
            assert ctx.velocity_planes() == (False, False, T if planes else 0, T)
            return snapshot(ctx)
        finally:
            ctx.close()
    assert same(run(True), run(False))
