"""The hard wall's taken branch in every kernel form that carries a copy of it, against helpers.hardwall_reference (np.longdouble).

The synthetic systems start their Drude particles 1.4e-4 nm from their parents; the 0.02 nm wall most GPU tests switch on is
140 sigma away and its branch never runs there.  Here every Drude particle is PUT where one rescale + half kick + drift takes its
pair across the wall (helpers.hot_wall_state), and single thermostat begins are compared -- a bounce is a discontinuity, and a
long trajectory through many of them compares nothing.  tests/test_hardwall.py asserts on the reference alone, for every case
below, that each class of pair is there, that every decision is far from its threshold and that a wrong wall would be seen.

Per step k the device runs setForces(f_k), step_begin, setForces(f_k+1), step_end (or the constraint path's four entry points);
the reference (helpers.wall_sequence) starts from what the device holds after setPositions / setVelocities / setForces, so the
representation of float, float + correction and the 2^32 fixed-point force is not charged to the kernels.  Forms whose own begin
is the second one (a deferred handle's first begin has nothing pending and is the plain kernel) run their first step without a
wall on a state built one drift further back, and the wall is switched on between the steps: no other way lets a pair START the
compared begin outside the wall.

Tolerances: helpers.hot_tolerances.  The bounce bound r <= max_dist (1 + 1e-6) of the reference's own test holds for every pair
whose Drude particle was moving away from its parent.  A pair caught outside with its Drude particle coming back is turned round
all the same (Ref :350: -dotvr1 / |dotvr1|) and leaves the wall at max_dist + deltaT vBond -- 1.0072 max_dist here, in the
reference as on the device; for those the test asserts that value instead.
"""
import numpy as np
import pytest

from openmm_drudenose_amd import _lib, synth
from openmm_drudenose_amd.drudetgnhplugin import (HipContext, TgnhError, FLAG_DEFER_SCALE, FLAG_RESIDENT_STEP, FLAG_WAVE_TILES,
                                                   FLAG_GATHER)
from helpers import (HOT_DT, HOT_FORMS, HOT_WALL, HotCase, hot_form_cases, hot_tolerances, hot_walls, oracle_run, rel_err,
                     wall_classes)

pytestmark = pytest.mark.gpu

assert (FLAG_DEFER_SCALE, FLAG_RESIDENT_STEP, FLAG_WAVE_TILES, FLAG_GATHER) == (2, 4, 8, 32)       # what helpers.HOT_FORMS spells out


def begin(ctx, split):
    if not split:
        return ctx.step_begin()
    for fn in (ctx.lib.tgnh_step_begin_kick, ctx.lib.tgnh_step_begin_move):      # Cu :351-360, :366-376; no constraint call-out between
        assert fn(ctx.h, ctx._stream()) == 0


def end(ctx, split):
    if not split:
        return ctx.step_end()
    for fn in (ctx.lib.tgnh_step_end_kick, ctx.lib.tgnh_step_end_thermo):
        assert fn(ctx.h, ctx._stream()) == 0


def install(ctx, hc):
    """the hot state -> what the device holds of it: positions, velocities, every force array"""
    ctx.setPositions(hc.pos)
    ctx.setVelocities(hc.vel)
    held = []
    for f in hc.forces:
        ctx.setForces(f)
        held.append(ctx.getForces())
    return ctx.getPositions(), ctx.getVelocities(), held


def run_steps(ctx, hc, walls, compared, split=False, kernel="unchecked"):
    """-> {k: (positions, velocities) directly after begin k}; the wall of every step is set before its begin"""
    out = {}
    for k, wall in enumerate(walls):
        if ctx.integrator.getMaxDrudeDistance() != wall:
            ctx.integrator.setMaxDrudeDistance(wall)
        if kernel != "unchecked":
            assert ctx.resident_kernel() == kernel
        ctx.setForces(hc.forces[k])
        begin(ctx, split)
        if k in compared:
            out[k] = (ctx.getPositions(), ctx.getVelocities())
        ctx.setForces(hc.forces[k + 1])
        end(ctx, split)
    return out


def launches(ctx, form, nsteps):
    """what the timing counters must say of `nsteps` steps of this form: a silent fall-back to another form is no coverage"""
    step, skd = ctx.timing_read(_lib.KID_STEP)[1], ctx.timing_read(_lib.KID_SKD)[1]
    if form == "step_kernel<STEP_PLAIN_BEGIN>":
        assert step == 2 * nsteps and skd == 0               # each thermostat half one launch of step_kernel
    elif form in ("step_kernel<STEP_DEFER>", "wstep_kernel"):
        assert step == nsteps - 1 and skd == 1               # the first begin: the plain tile launch; then one launch per step
    elif form.startswith("tile_kernel") and "MOVE" not in form:
        assert step == 0 and skd == nsteps
    else:
        assert step == 0


def errors(got, ref, members):
    (p, v), rp, rv = got, ref["pos"], ref["vel"]
    return rel_err(p, rp), rel_err(v, rv), rel_err(p[members], rp[members]), rel_err(v[members], rv[members])


def check_bounces(hc, got, ref, wall=HOT_WALL, kT_drude=None, single=False):
    """the bounce bound, and the value the reference's arithmetic gives where the bound cannot hold (module docstring); float32
    positions hold a distance to 4 x 2^-24 max|x| (two particles, rounded per coordinate), i.e. to that times kappa of the wall"""
    s, info = hc.system, ref["info"]
    r = np.linalg.norm(got[0][s.pair_drude] - got[0][s.pair_parent], axis=1)
    away = info["out"] & (info["dotvr1"] > 0)
    back = info["out"] & (info["dotvr1"] < 0)
    assert (away | back | ~info["out"]).all()
    assert r[away].max() <= wall * (1 + 1e-6)
    if back.any():
        kT = synth.KB * hc.drude_temperature if kT_drude is None else kT_drude
        deltaT = np.minimum(info["dt_raw"][back], 1.0) * HOT_DT
        assert np.allclose(r[back], wall + deltaT * np.sqrt(kT / s.mass[s.pair_drude][back]), rtol=max(1e-6, 4 * 2.0 ** -24 * hc.kappa * single), atol=0)


@pytest.mark.parametrize("form,sysname,mode,chains,precision", hot_form_cases())
def test_hard_wall_form(form, sysname, mode, chains, precision):
    d = HOT_FORMS[form]
    hc = HotCase(sysname, mode, chains, d["delay"])
    walls, compared = hot_walls(d["delay"], precision)
    flags = 0 if sysname == "far" else d["flags"]               # (far_pairs: on the gather path by its topology, not by asking)
    ctx = HipContext(hc.system, hc.make_integrator(walls[0]), mode=mode, precision=precision, flags=flags)
    try:
        assert ctx.step_path()[0] == d["path"] and ("asked for" in ctx.step_path()[1]) == (flags == FLAG_GATHER)
        pos0, vel0, forces = install(ctx, hc)
        ctx.timing(True)
        got = run_steps(ctx, hc, walls, compared, d["split"], d["kernel"])
        ctx.torch.cuda.synchronize()
        ctx.timing(False)
        launches(ctx, form, len(walls))
        assert ctx.check() == 0                                  # (bits 3 and 4 among them: no meeting timed out)
    finally:
        ctx.close()
    ref = hc.reference(walls, pos0, vel0, forces)
    tol = hot_tolerances(precision, hc.kappa)
    for k in compared:
        info = ref[k]["info"]
        classes = wall_classes(info)
        e = errors(got[k], ref[k], hc.members(info["out"]))
        print(f"{form} {sysname} {mode} {chains} {precision} begin {k + 1}: {int(info['out'].sum())} of {len(info['out'])} pairs bounced, "
              f"pos {e[0]:.2e} vel {e[1]:.2e}, bounced pairs alone pos {e[2]:.2e} vel {e[3]:.2e} (tolerance {tol[0]:.1e} / {tol[1]:.1e})")
        assert info["out"].sum() >= 3 and all(classes[c].sum() >= 3 for c in ("inside", "free"))
        assert e[0] <= tol[0] and e[2] <= tol[0] and e[1] <= tol[1] and e[3] <= tol[1]
        check_bounces(hc, got[k], ref[k], single=precision == "single")
    # what the wall does not move it must not perturb: the same begin from a handle that never has a wall, bit for bit
    k = compared[0]
    ctx = HipContext(hc.system, hc.make_integrator(0.0), mode=mode, precision=precision, flags=flags)
    try:
        install(ctx, hc)
        free = run_steps(ctx, hc, (0.0,) * (k + 1), (k,), d["split"])[k]
    finally:
        ctx.close()
    moved = np.zeros(hc.system.num_particles, bool)
    moved[hc.members(ref[k]["info"]["out"])] = True
    assert np.array_equal(got[k][0][~moved], free[0][~moved]) and np.array_equal(got[k][1][~moved], free[1][~moved])
    assert not np.array_equal(got[k][1][moved], free[1][moved])


BEYOND = [("tile_kernel<S|K|D>", 0), ("step_kernel<STEP_PLAIN_BEGIN>", 0), ("wstep_kernel", 1), ("gather_update_kernel", 0)]


@pytest.mark.parametrize("mode", ["TGNH", "dualNH"])
@pytest.mark.parametrize("form,delay", BEYOND)
def test_beyond_twice_the_wall(form, delay, mode):
    """One pair past 2 x max_dist after the drift (2.4 x: the margin is the reference's to show).  TGNH: status bit 0, no error (K has
    no throw), and the result is the reference's, which bounces that pair like any other.  dualNH: TGNH_ERR_HARDWALL, for good."""
    d = HOT_FORMS[form]
    hc = HotCase("water27", mode, 1, delay, beyond=5)
    walls, compared = hot_walls(delay, "double")
    walls, compared = walls[:compared[0] + 1], compared[:1]
    ctx = HipContext(hc.system, hc.make_integrator(walls[0]), mode=mode, precision="double", flags=d["flags"])
    try:
        assert ctx.step_path()[0] == d["path"]
        pos0, vel0, forces = install(ctx, hc)
        ref = hc.reference(walls, pos0, vel0, forces)[compared[0]]
        ratio = ref["info"]["ratio"]
        assert ratio[5] > 2.2 and np.delete(ratio, 5).max() < 1.9
        got = run_steps(ctx, hc, walls, compared, d["split"], d["kernel"])[compared[0]]
        if mode == "TGNH":
            assert ctx.check() == 1 and ctx.status_flags() == 1
            e = errors(got, ref, hc.members(ref["info"]["out"]))
            print(f"beyond twice the wall, {form}: pos {e[0]:.2e} vel {e[1]:.2e}, bounced pairs alone pos {e[2]:.2e} vel {e[3]:.2e}")
            assert max(e) <= 1e-12
        else:
            for _ in range(2):                                   # sticky: every later query and step fails too
                with pytest.raises(TgnhError, match="too far beyond hard wall") as err:
                    ctx.check()
                assert err.value.status == _lib.ERR_HARDWALL
            with pytest.raises(TgnhError, match="too far beyond hard wall"):
                ctx.step_begin()
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["TGNH", "dualNH"])
@pytest.mark.parametrize("flags,kernel", [(0, None), (FLAG_RESIDENT_STEP, "step_kernel"), (FLAG_WAVE_TILES, None),
                                           (FLAG_RESIDENT_STEP | FLAG_WAVE_TILES, "step_kernel")])
def test_wall_switched_on_and_off_in_a_live_handle(flags, kernel, mode):
    """Created without a wall, two steps, then the wall and a hot state: the launch's LDS size and its grid-cache / resident_grid
    entry change.  Same agreement as in a fresh handle; then off again, and a further begin is the reference's without a wall.
    (The handles whose velocities lag between steps refuse a new state there: their wall is switched on in test_hard_wall_form.)"""
    hc = HotCase("water27", mode, 1, 0, wall=0.0)
    ctx = HipContext(hc.system, hc.make_integrator(0.0), mode=mode, precision="double", flags=flags)
    try:
        o = hc.oracle()
        oracle_run(o, hc.system, 2, x0=ctx.sites())
        ctx.step(2)
        assert ctx.resident_kernel() == kernel
        pos0, vel0, forces = install(ctx, hc)
        walls = (HOT_WALL, 0.0)
        got = run_steps(ctx, hc, walls, (0, 1), False, kernel)
        assert ctx.check() == 0
    finally:
        ctx.close()
    ref = hc.reference(walls, pos0, vel0, forces, oracle=o)
    for k in (0, 1):
        mem = hc.members(ref[0]["info"]["out"])
        e = errors(got[k], ref[k], mem)
        print(f"live handle flags {flags} {mode}, wall {'on' if walls[k] else 'off again'}: pos {e[0]:.2e} vel {e[1]:.2e}, bounced pairs alone pos {e[2]:.2e} vel {e[3]:.2e}")
        assert max(e) <= 1e-12
    assert ref[0]["info"]["out"].sum() >= 3
    check_bounces(hc, got[0], ref[0])
    r = np.linalg.norm(got[1][0][hc.system.pair_drude] - got[1][0][hc.system.pair_parent], axis=1)
    assert (r > HOT_WALL).sum() >= 3                                 # the wall is off: the late pairs cross and stay out


@pytest.mark.parametrize("mode", ["TGNH", "dualNH"])
@pytest.mark.parametrize("form", ["tile_kernel<S|K|D>", "step_kernel<STEP_PLAIN_BEGIN>", "wstep_kernel", "gather_update_kernel"])
def test_retargeted_drude_bath_sets_the_bounce_speed(form, mode):
    """setDrudeTemperature(25) on a live handle: the bounce leaves at sqrt(kB 25 K / m), five times the speed it was created with
    (tests/test_hardwall.py: the reference at the wrong temperature is > 100 tolerances away)."""
    d = HOT_FORMS[form]
    hc = HotCase("water27", mode, 1, d["delay"])
    walls, compared = hot_walls(d["delay"], "double")
    it = hc.make_integrator(walls[0])
    ctx = HipContext(hc.system, it, mode=mode, precision="double", flags=d["flags"])
    try:
        it.setDrudeTemperature(25.0)
        hc.drude_temperature, hc.integrator = 25.0, it                # the oracle and the reference wall: at the new temperature
        pos0, vel0, forces = install(ctx, hc)
        got = run_steps(ctx, hc, walls, compared, d["split"], d["kernel"])
        assert ctx.check() == 0
    finally:
        ctx.close()
    ref = hc.reference(walls, pos0, vel0, forces)
    for k in compared:
        e = errors(got[k], ref[k], hc.members(ref[k]["info"]["out"]))
        print(f"Drude bath retargeted to 25 K, {form} {mode} begin {k + 1}: pos {e[0]:.2e} vel {e[1]:.2e}, bounced pairs alone pos {e[2]:.2e} vel {e[3]:.2e}")
        assert ref[k]["info"]["out"].sum() >= 3 and max(e) <= 1e-12
        check_bounces(hc, got[k], ref[k])
