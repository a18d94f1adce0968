"""The velocity planes hold the massive slots only (tgnh_topology.cpp, tgnh_wave_device.h): a massless slot -- one in
five of an SWM4 water box -- has no word in them, its register image is (0, 0, 0, w = 0), and its x, y, z in velm are left alone
by both conversions.  Every comparison here is what tests/test_velocity_planes_gpu.py's are: the same call sequence on a handle
created with TGNH_VELOCITY_PLANES=0, bit for bit (positions, velocities after a settle, thermostat state, kinetic energies), and
every run takes more than 8 + 12 steps with the planes asserted live.  That file's sequences are used as they stand (steady_run:
24 steps, the hard wall switched on and taken once the planes are live); what is new here are the boxes -- those of
tests/test_velocity_planes_layout.py, where the indexing base[tile] + offset[lane] can go wrong: the massless slot last or fourth
of five, two of them, none, tiles of another pattern, a trailing tile of one to five molecules -- and what a massless slot's velm
words may hold.

tgnh_algorithmic_bytes(KID_STEP) is not asserted here: tests/test_velocity_planes_gpu.py pins it to 3 x 24 B of V per slot on
the planes for the same water boxes, so the query still counts the full planes (DESIGN.md 4 says by how much that overstates
the launch)."""
import numpy as np
import pytest

from openmm_drudenose_amd.drudetgnhplugin import TgnhError
from helpers import make_oracle, oracle_run, rel_err
from massive_planes_boxes import NAMES, box
from test_velocity_planes_gpu import T, context, live, one_launch_grid, same, snapshot, steady_run

pytestmark = pytest.mark.gpu


def bits(arrays):
    """for runs that hold NaNs: the comparison of bit patterns"""
    return [np.ascontiguousarray(a, np.float64).view(np.uint64) for a in arrays]


def on_and_off(name, mode, precision, chains, share=None, inspect=None):
    kw = dict(system=box(name), share=share)
    on = steady_run(0, mode, precision, chains, True, inspect=inspect, **kw)
    off = steady_run(0, mode, precision, chains, False, **kw)
    assert on[3] == off[3]
    assert np.array_equal(on[0], off[0]), "positions differ after the first step with the wall"
    assert same(on[1], off[1]), "an odd number of steps"
    assert same(on[2], off[2]), "an even number of steps"
    return on


@pytest.mark.parametrize("mode", ["TGNH", "dualNH"])
@pytest.mark.parametrize("chains", [1, 3])
@pytest.mark.parametrize("precision", ["mixed", "double"])
@pytest.mark.parametrize("name", NAMES)
def test_steps_on_the_compact_planes_are_the_steps_on_velm(name, precision, chains, mode):
    on_and_off(name, mode, precision, chains)


def test_the_wall_was_taken_on_the_compact_planes():
    """... on the box whose Drude particle sits behind the massless slot: the same steps without a wall end elsewhere"""
    on = on_and_off("nacl-order", "TGNH", "mixed", 1)
    free = steady_run(0, "TGNH", "mixed", 1, True, with_wall=False, system=box("nacl-order"))
    assert free[3] == on[3] and not np.array_equal(free[0], on[0])


# ---------------------------------------------------------------------------------------------------------------------
# several tiles per wavefront: the held tile, the way back, the refetch of word, 1/m and OFFSET at a new pattern word, the
# trailing tile of five molecules
# ---------------------------------------------------------------------------------------------------------------------
_WALK_BOXES = {}


def walk_box(name):
    if name not in _WALK_BOXES:
        from helpers import water_row
        _WALK_BOXES[name] = box("water1001") if name == "water1001" else water_row("mod5", 3000)
    return _WALK_BOXES[name]


@pytest.mark.parametrize("share", [64, 1])
@pytest.mark.parametrize("name,precision,chains", [("water1001", "mixed", 1), ("water1001", "double", 1), ("water1001", "mixed", 3),
                                                   ("mod5-3000", "mixed", 1), ("mod5-3000", "double", 1), ("mod5-3000", "mixed", 3)])
def test_a_wavefront_walks_several_tiles_on_the_compact_planes(name, precision, chains, share):
    """tgnh_set_resident_share(64): 84 (250) wave tiles on 8 work-groups, or 4 with a chain of three links -- some (all) wavefronts
    hold more than one tile, the last of them the 25-slot (60-slot) tile the box ends with; in the mod5 box every hop meets
    another pattern word.  Share 1: one tile per wavefront."""
    def walk(ctx):
        nw, grid = one_launch_grid(ctx, share)
        print(f"{name} {precision} chains={chains} share={share}: {nw} wave tiles on {grid} work-groups")
        assert (nw > 8 * grid) == (share == 64)
    kw = dict(system=walk_box(name), share=share)
    on = steady_run(0, "TGNH", precision, chains, True, inspect=walk, **kw)
    off = steady_run(0, "TGNH", precision, chains, False, **kw)
    assert on[3] == off[3] and np.array_equal(on[0], off[0]) and same(on[1], off[1]) and same(on[2], off[2])


# ---------------------------------------------------------------------------------------------------------------------
# what a massless slot's x, y, z in velm may hold
# ---------------------------------------------------------------------------------------------------------------------
def junk_for(ctx, massless):
    """finite, non-zero, of either sign, no two alike"""
    k = np.arange(3 * len(massless), dtype=np.float64).reshape(-1, 3)
    return ctx.torch.tensor((-1.0) ** k * (0.25 + k / 7.0), dtype=ctx.velm.dtype, device=ctx.velm.device)


@pytest.mark.parametrize("name", ["water13", "nacl-order", "two-massless"])
@pytest.mark.parametrize("precision", ["mixed", "double"])
def test_finite_numbers_in_the_massless_slots_stay_where_they_are(name, precision):
    s = box(name)[0]
    massless = np.flatnonzero(s.mass == 0.0)
    assert len(massless) > 0

    def run(planes):
        ctx = context(box(name), planes, precision=precision, wall=0.02)
        try:
            idx = ctx.torch.as_tensor(massless, device=ctx.velm.device)
            junk = junk_for(ctx, massless)
            ctx.velm[idx, :3] = junk
            ctx.step(T + 4)
            assert live(ctx) == planes and ctx.time()[1] == T + 4
            out = snapshot(ctx)                              # (the velocity read-back settles: the planes are left)
            assert not live(ctx)
            assert np.array_equal(ctx.velm[idx, :3].cpu().numpy(), junk.cpu().numpy()), "a massless slot's velm words were touched"
            assert np.all(ctx.velm[idx, 3].cpu().numpy() == 0.0)
            ctx.step(T + 4)                                  # ... and a second stay
            assert live(ctx) == planes
            out += snapshot(ctx)
            assert np.array_equal(ctx.velm[idx, :3].cpu().numpy(), junk.cpu().numpy())
            assert ctx.check() == 0
            return out
        finally:
            ctx.close()
    assert same(run(True), run(False))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("precision", ["mixed", "double"])
def test_a_massless_slot_that_is_not_finite_keeps_the_handle_on_velm(bad, precision):
    """the full planes carried such a word into the molecule's momentum sum as NaN * 0, the compact planes would not: the entry
    check finds it, with the verdict of a w that is not its table entry, and the handle does what the handle with the switch
    off does.  That is: NaN kinetic energies from the first step on, which the library reports as a failure once it reads its
    status word (measured: at step 21) -- so what is compared is everything that can be read on the way there, bit for bit,
    and how each call ends."""
    s = box("water1001")[0]
    slot = 5 * 417 + 4                                       # an M site in the middle of the box
    assert s.mass[slot] == 0.0

    def attempt(fn):
        try:
            out = fn()
            return bits(out) if isinstance(out, list) else [] if out is None else bits([out])
        except TgnhError as e:
            return [("failed", e.status)]

    def run(planes):
        ctx = context(box("water1001"), planes, precision=precision, wall=0.02)
        try:
            v = ctx.getVelocities()
            v[slot, 1] = bad
            ctx.setVelocities(v)                             # through the API
            got = ctx.velm[slot].cpu().numpy()
            assert not np.isfinite(got[1]) and got[3] == 0.0
            ctx.step(T + 1)
            assert ctx.velocity_planes() == (False, planes, T if planes else 0, T)
            ctx.step(4)                                      # the conversion ran, found the slot, and was dropped
            assert ctx.velocity_planes() == (False, False, T if planes else 0, T)
            out = attempt(ctx.getPositions)
            out += attempt(lambda: ctx.step(T))
            assert not live(ctx) and ctx.velocity_planes()[1] is False
            out += attempt(lambda: snapshot(ctx))
            return out
        finally:
            ctx.close()
    on, off = run(True), run(False)
    print(f"{precision} {bad}: {len(on)} records, of them calls that failed: {[r for r in on if isinstance(r, tuple)]}")
    assert same(on, off)


# ---------------------------------------------------------------------------------------------------------------------
# transitions, on the box where a lane's offset is not lane - lane div 5
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["mixed", "double"])
def test_a_read_back_and_a_flush_in_the_middle_of_a_run(precision):
    def run(planes):
        ctx = context(box("nacl-order"), planes, precision=precision, wall=0.02)
        try:
            ctx.step(T + 4)
            assert live(ctx) == planes
            out = [ctx.getVelocities()]
            assert not live(ctx)
            ctx.step(T + 4)
            assert live(ctx) == planes
            ctx.flush()
            assert not live(ctx)
            out.append(ctx.velm.cpu().numpy())
            ctx.step(T)                                      # a plain begin and T - 1 one-launch steps: still on velm
            assert ctx.velocity_planes() == (False, planes, T - 1 if planes else 0, T)
            ctx.step(T)
            assert live(ctx) == planes and ctx.time()[1] == 4 * T + 8
            out += snapshot(ctx)
            assert ctx.check() == 0
            return out
        finally:
            ctx.close()
    assert same(run(True), run(False))


def test_a_checkpoint_restored_into_a_fresh_handle():
    def run(planes):
        a = context(box("nacl-order"), planes, wall=0.02)
        b = None
        try:
            a.step(14)
            assert live(a) == planes
            pos, vel, clock = a.getPositions(), a.getVelocities(), a.time()
            assert not live(a)
            thermo = [a.thermostat_state(w) for w in range(3)]
            b = context(box("nacl-order"), planes, wall=0.02)
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


def test_velm_rebound_inside_a_step():
    """the array that goes gets the velocities back first -- its massless slots as they were --, and the first conversion of
    the new bind checks the new array: w against the table, the massless slots' x, y, z for finite numbers"""
    def run(planes):
        ctx = context(box("nacl-order"), planes, wall=0.02)
        try:
            ctx.step(T + 3)
            assert live(ctx) == planes
            ctx.step_begin()
            ctx.compute_forces()
            fresh = ctx.velm.clone()
            old = ctx.rebind_velocities(fresh)
            assert ctx.velm is fresh and ctx.velocity_planes() == (False, planes, 0, T)
            current = old.cpu().numpy()
            fresh.copy_(old)
            ctx.step_end()
            ctx.step(T + 1)
            assert ctx.velocity_planes() == (planes, planes, T + 1 if planes else 0, T)
            ctx.step(2)
            out = snapshot(ctx) + [current]
            assert ctx.check() == 0
            return out
        finally:
            ctx.close()
    assert same(run(True), run(False))


# ---------------------------------------------------------------------------------------------------------------------
# ... and against the oracle
# ---------------------------------------------------------------------------------------------------------------------
TOL = 1e-6           # tests/test_gpu_parity.py's figure for positions and velocities after up to 100 steps of 1 fs


def test_steps_on_the_compact_planes_against_the_oracle():
    s, g, ng = box("nacl-order")
    ctx = context((s, g, ng), True, "TGNH", "mixed", 1, wall=0.02, dt=0.001)
    try:
        assert ctx.resident_kernel() == "wstep_kernel" and ctx.velocity_planes()[1]
        x0 = ctx.sites()
        pos_o, vel_o = oracle_run(make_oracle(s, g, ng, "TGNH", ctx.integrator), s, 30, x0=x0)
        ctx.step(30)
        assert live(ctx)
        ep, ev = rel_err(ctx.getPositions(), pos_o), rel_err(ctx.getVelocities(), vel_o)
        print(f"nacl-order, 30 steps on the compact planes against the oracle: pos {ep:.2e} vel {ev:.2e}")
        assert ctx.check() == 0
        assert ep <= TOL and ev <= TOL, (ep, ev)
    finally:
        ctx.close()
