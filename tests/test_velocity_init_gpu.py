"""GPU tests of tgnh_set_velocities_to_temperature (tgnh_velinit.hip) and tgnh_set_temperatures.

The velocities are held against `draw` of tests/test_velocity_init.py: the header's specification restated in numpy.  The bound of
the exact draw is derived, not measured: a velocity is a chain of about six fp64 operations behind few-ulp log, sin, cos on
|z| <= 6.8, i.e. some 1e-14 of the slot's thermal speed sigma; 1e-12 sigma leaves two orders of margin.  In single precision
the fp64 value is rounded once to float: 2^-23 |v| on top."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import (DrudeTGNHIntegrator, HipContext, TgnhError, create_handle, FLAG_DEFER_SCALE,
                                                   FLAG_WAVE_TILES, FLAG_TRUST_STATE_CHANGED, FLAG_GATHER)
from test_velocity_init import draw, inverse_masses, STAT_SEEDS

pytestmark = pytest.mark.gpu

SYSTEMS = {"pair+normal+massless": synth.pair_normal_massless,
           "nacl": synth.nacl,                               # 2 500 slots in five tiles; the Drude last in a water, ions among waters
           "water216": lambda: synth.water_box(216)}         # 1 080 slots, wave tiles
_cache = {}


def system(name):
    if name not in _cache:
        _cache[name] = SYSTEMS[name]()[0]
    return _cache[name]


def integ(temperature=300.0, drude_temperature=1.0, chains=3, drude_chains=True, hardwall=0.0):
    it = DrudeTGNHIntegrator(temperature, 0.1, drude_temperature, 0.005, 0.001, 20, chains, drude_chains, True)
    it.setMaxDrudeDistance(hardwall)
    return it


def context(s, mode="TGNH", precision="mixed", flags=0, **kw):
    return HipContext(s, integ(**kw), mode=mode, precision=precision, flags=flags)


def velocities(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    return ctx.velm[:, :3].cpu().numpy()


def call(ctx, temperature, drude_temperature, seed, first=0):
    return ctx.lib.tgnh_set_velocities_to_temperature(ctx.h, temperature, drude_temperature, seed, first, ctx._stream())


# ---- 1. the exact draw
@pytest.mark.parametrize("precision", ["double", "mixed", "single"])
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_exact_draw(name, precision):
    s = system(name)
    ctx = context(s, precision=precision)
    ctx.torch.cuda.synchronize(ctx.dev)
    w0 = ctx.velm[:, 3].clone()
    pos0 = [ctx.posq.clone(), None if ctx.posq_corr is None else ctx.posq_corr.clone()]
    ctx.setVelocitiesToTemperature(300.0, 20191024, 1.0)
    v = velocities(ctx).astype(np.float64)
    w = inverse_masses(s, precision)
    assert np.array_equal(w0.cpu().numpy().astype(np.float64), w)          # (the yardstick reads the masses the kernel reads)
    ref, sigma = draw(w, s.pair_drude, s.pair_parent, 300.0, 1.0, 20191024)
    bound = 1e-12 * sigma[:, None] + (2.0 ** -23 * np.abs(ref) if precision == "single" else 0.0)
    err = np.abs(v - ref)
    print(f"{name} {precision}: max |dv| / sigma = {(err[sigma > 0] / sigma[sigma > 0, None]).max():.3e}")
    assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
    assert (v[s.mass == 0.0] == 0.0).all() and (s.mass == 0.0).any()
    assert np.abs(v[s.mass > 0]).min() > 0
    assert ctx.torch.equal(ctx.velm[:, 3], w0)                             # w bit for bit
    assert ctx.torch.equal(ctx.posq, pos0[0]) and (pos0[1] is None or ctx.torch.equal(ctx.posq_corr, pos0[1]))
    ctx.close()


# ---- 2. one draw whatever the path
@pytest.mark.parametrize("name", ["nacl", "water216"])
def test_one_draw_whatever_the_path(name):
    s = system(name)
    want, paths = None, set()
    for mode in ("TGNH", "dualNH"):
        for flags in (0, FLAG_WAVE_TILES, FLAG_GATHER):
            ctx = context(s, mode=mode, flags=flags)
            paths.add(ctx.step_path()[0])
            ctx.setVelocitiesToTemperature(300.0, 4242, 1.0)
            v = velocities(ctx)
            want = v if want is None else want
            assert v.tobytes() == want.tobytes(), (mode, flags)
            ctx.close()
    assert paths == {"tiled", "gather"}


# ---- 3. one draw whatever the sharding
def test_one_draw_whatever_the_sharding():
    s = system("water216")
    cut = 5 * 100                                            # molecule 100: slot 500, not a multiple of 64
    assert cut % 64 != 0
    whole = context(s)
    whole.setVelocitiesToTemperature(300.0, 77, 1.0)
    want = velocities(whole)
    whole.close()
    parts = []
    for lo, hi in ((0, cut), (cut, s.num_particles)):
        ctx = context(s.slice_molecules(lo, hi))
        ctx.first_particle = lo
        ctx.setVelocitiesToTemperature(300.0, 77, 1.0)
        parts.append(velocities(ctx))
        ctx.close()
    assert np.concatenate(parts).tobytes() == want.tobytes()


# ---- 4. seeds
def test_seeds():
    ctx = context(system("nacl"))
    ctx.setVelocitiesToTemperature(300.0, 5, 1.0)
    a = velocities(ctx)
    ctx.setVelocitiesToTemperature(300.0, 6, 1.0)
    b = velocities(ctx)
    ctx.setVelocitiesToTemperature(300.0, 5 + (1 << 32), 1.0)              # the seed's high word
    c = velocities(ctx)
    ctx.setVelocitiesToTemperature(300.0, 5, 1.0)
    assert velocities(ctx).tobytes() == a.tobytes()
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    ctx.first_particle = 1
    ctx.setVelocitiesToTemperature(300.0, 5, 1.0)
    assert not np.array_equal(velocities(ctx), a)
    ctx.first_particle = 0
    ctx.setVelocitiesToTemperature(300.0)                                  # a seed from os.urandom, the integrator's Drude temperature
    assert not np.array_equal(velocities(ctx), a)
    ctx.setVelocitiesToTemperature(0.0, 5, 0.0)
    z = velocities(ctx)
    assert (z == 0).all() and not np.signbit(z).any()
    ctx.close()


# ---- 5. temperatures land where the thermostats look
@pytest.mark.parametrize("seed", STAT_SEEDS)
def test_temperatures_land_where_the_thermostats_look(seed):
    """The kinetic energy of a Gaussian draw is chi^2 with n_i degrees of freedom: relative sigma sqrt(2 / n_i); five of them
    (the yardstick alone sits within four for these seeds: tests/test_velocity_init.py)."""
    s = synth.water_box(4096)[0]
    ctx = context(s)
    dof, _ = ctx.dof()
    ctx.setVelocitiesToTemperature(300.0, seed, 1.0)
    t = ctx.compute_kinetic_energies() / dof / synth.KB
    dev = np.abs(t / np.array([300.0, 300.0, 1.0]) - 1.0)
    print(f"seed {seed}: T = {t}, |T / target - 1| = {dev}, allowed {5 * np.sqrt(2 / dof)}")
    assert (dev <= 5.0 * np.sqrt(2.0 / dof)).all()
    ctx.close()


# ---- 6. state
def test_refused_like_state_changed_inside_a_deferred_sequence():
    """Between two steps of a TGNH_FLAG_DEFER_SCALE handle the call answers what tgnh_state_changed answers there, and velm is
    untouched.  tgnh_flush brings velm up to date but does not take back the thermostat half that has already run: on such a
    handle tgnh_state_changed -- and so this call -- stays refused after it (asserted as "the same answer"); where
    tgnh_state_changed is accepted (the same handle before its first step, a handle without the flag after a flush) the call
    succeeds."""
    s = system("nacl")
    ctx = context(s, flags=FLAG_DEFER_SCALE)
    assert call(ctx, 300.0, 1.0, 3) == _lib.TGNH_OK          # nothing owed yet
    ref, _ = draw(inverse_masses(s, "mixed"), s.pair_drude, s.pair_parent, 300.0, 1.0, 3)
    assert np.abs(velocities(ctx) - ref).max() < 1e-12
    ctx.step(2)
    ctx.torch.cuda.synchronize(ctx.dev)
    before = ctx.velm.clone()
    refused = ctx.lib.tgnh_state_changed(ctx.h)
    assert refused == _lib.ERR_STATE
    assert call(ctx, 300.0, 1.0, 3) == refused
    with pytest.raises(TgnhError):
        ctx.setVelocitiesToTemperature(300.0, 3)
    ctx.torch.cuda.synchronize(ctx.dev)
    assert ctx.torch.equal(ctx.velm, before)
    assert ctx.lib.tgnh_flush(ctx.h, ctx._stream()) == _lib.TGNH_OK
    ctx.torch.cuda.synchronize(ctx.dev)
    flushed = ctx.velm.clone()
    assert not ctx.torch.equal(flushed, before)
    after = ctx.lib.tgnh_state_changed(ctx.h)
    assert call(ctx, 300.0, 1.0, 3) == after
    ctx.torch.cuda.synchronize(ctx.dev)
    assert after == _lib.TGNH_OK or ctx.torch.equal(ctx.velm, flushed)
    ctx.close()
    plain = context(s)
    plain.step(2)
    assert plain.lib.tgnh_flush(plain.h, plain._stream()) == _lib.TGNH_OK
    assert call(plain, 300.0, 1.0, 3) == _lib.TGNH_OK
    assert np.abs(velocities(plain) - ref).max() < 1e-12
    plain.close()


def test_a_carried_kinetic_energy_is_dropped():
    """TGNH_FLAG_TRUST_STATE_CHANGED: after the call pending bit 9 is clear, and the next step's kinetic energies are those of
    a twin that was given the same velocities through setVelocities"""
    s = system("nacl")
    a, b = context(s, flags=FLAG_TRUST_STATE_CHANGED), context(s, flags=FLAG_TRUST_STATE_CHANGED)
    a.step(3)
    b.step(3)
    assert a.pending_state() & 0x200 and b.pending_state() & 0x200
    a.setVelocitiesToTemperature(300.0, 11, 1.0)
    assert not a.pending_state() & 0x200 and not a.ke_sum_valid
    b.setVelocities(velocities(a).astype(np.float64))
    a.step_begin()
    b.step_begin()
    ka, kb = a.last_kinetic_energies(), b.last_kinetic_energies()
    assert ka.tobytes() == kb.tobytes() and (ka[[0, 1, 2]] > 0).all()
    a.compute_forces(); b.compute_forces()
    a.step_end(); b.step_end()
    assert a.last_kinetic_energies().tobytes() == b.last_kinetic_energies().tobytes()
    a.close()
    b.close()


def test_errors():
    s = system("nacl")
    ctx = context(s)
    ctx.torch.cuda.synchronize(ctx.dev)
    before = ctx.velm.clone()
    for t, td, first in ((-1.0, 1.0, 0), (300.0, -1e-9, 0), (np.nan, 1.0, 0), (300.0, np.inf, 0), (300.0, 1.0, -1)):
        assert call(ctx, t, td, 1, first) == _lib.ERR_ARG, (t, td, first)
    assert ctx.lib.tgnh_set_velocities_to_temperature(None, 300.0, 1.0, 1, 0, ctx._stream()) == _lib.ERR_ARG
    ctx.torch.cuda.synchronize(ctx.dev)
    assert ctx.torch.equal(ctx.velm, before)
    # buffers not bound
    it = integ()
    group, ngroups = it._resolve_groups(s.num_particles)
    h = create_handle(ctx.lib, s, it, group, ngroups, _lib.MODE_TGNH, _lib.PREC_MIXED, 0, 0, synth.KB, ctx.padded)
    assert ctx.lib.tgnh_set_velocities_to_temperature(h, 300.0, 1.0, 1, 0, ctx._stream()) == _lib.ERR_STATE
    assert ctx.lib.tgnh_destroy(h) == _lib.TGNH_OK
    ctx.close()


# ---- 7. retargeting is a handle created there
def state_bits(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    out = [ctx.posq.cpu().numpy().tobytes(), ctx.velm.cpu().numpy().tobytes()]
    if ctx.posq_corr is not None:
        out.append(ctx.posq_corr.cpu().numpy().tobytes())
    out += [ctx.thermostat_state(k).tobytes() for k in range(4)]
    out.append(ctx.last_scale_factors().tobytes())
    return out


@pytest.mark.parametrize("mode,drude_chains", [("TGNH", True), ("dualNH", False)])
def test_retargeting_is_a_handle_created_there(mode, drude_chains):
    s = system("nacl")
    kw = dict(chains=3, drude_chains=drude_chains, hardwall=0.02)
    a = context(s, mode=mode, **kw)
    a.step(20)
    assert a.lib.tgnh_set_temperatures(a.h, 350.0, 2.0, a._stream()) == _lib.TGNH_OK
    b = context(s, mode=mode, temperature=350.0, drude_temperature=2.0, **kw)
    assert a.dof()[1].tobytes() == b.dof()[1].tobytes()                    # tgnh_get_dof reports the new N kT
    assert not np.array_equal(a.dof()[1], context_nkt_at_300(s, mode, kw))
    # b: a restored checkpoint of a
    a.torch.cuda.synchronize(a.dev)
    b._state_changed()
    b.posq.copy_(a.posq)
    b.velm.copy_(a.velm)
    if a.posq_corr is not None:
        b.posq_corr.copy_(a.posq_corr)
    for k in range(4):
        b.set_thermostat_state(k, a.thermostat_state(k))
    b.set_time(*a.time())
    b.compute_forces()
    # c: the Python setters instead of the ABI call
    c = context(s, mode=mode, **kw)
    c.step(20)
    c.integrator.setTemperature(350)
    c.integrator.setDrudeTemperature(2)
    a.step(20)
    b.step(20)
    c.step(20)
    sa, sb, sc = state_bits(a), state_bits(b), state_bits(c)
    assert sa == sb
    assert sa == sc
    assert (a.check() & ~1) == 0                               # (bit 0: a Drude beyond twice the wall is a failure in dualNH only, and none happened)
    for ctx in (a, b, c):
        ctx.close()


def context_nkt_at_300(s, mode, kw):
    ctx = context(s, mode=mode, **kw)
    nkt = ctx.dof()[1]
    ctx.close()
    return nkt


def test_retargeting_refusals():
    s = system("nacl")
    ctx = context(s, flags=FLAG_DEFER_SCALE)
    assert ctx.lib.tgnh_set_temperatures(ctx.h, np.nan, 1.0, ctx._stream()) == _lib.ERR_ARG
    assert ctx.lib.tgnh_set_temperatures(ctx.h, 300.0, -2.0, ctx._stream()) == _lib.ERR_ARG
    ctx.step(2)
    nkt = ctx.dof()[1]
    assert ctx.lib.tgnh_state_changed(ctx.h) == _lib.ERR_STATE
    assert ctx.lib.tgnh_set_temperatures(ctx.h, 350.0, 2.0, ctx._stream()) == _lib.ERR_STATE       # mid-deferred-sequence
    with pytest.raises(TgnhError):
        ctx.integrator.setTemperature(350)
    assert ctx.integrator.getTemperature() == 300.0 and ctx.dof()[1].tobytes() == nkt.tobytes()
    ctx.close()


class CountingLib:
    """the library, counting the calls of every entry point"""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*args):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args)
        return counted


def test_a_run_that_never_retargets_never_calls_the_setter():
    s = system("nacl")
    ctx = context(s)
    ctx.lib = lib = CountingLib(ctx.lib)
    ctx.integrator.setStepSize(0.0005)                       # (pushes the scalars)
    ctx.integrator.setMaxDrudeDistance(0.02)
    ctx.integrator.setTemperature(300.0)                     # the value the handle runs at: nothing to push
    ctx.step(5)
    ctx.getVelocities()
    assert lib.calls.get("tgnh_set_step_size", 0) >= 2 and "tgnh_set_temperatures" not in lib.calls
    replay = ctx.capture_steps(2)
    replay()
    ctx.integrator.setTemperature(310.0)
    assert lib.calls["tgnh_set_temperatures"] == 1
    with pytest.raises(TgnhError, match="capture them again"):      # a recorded step holds the old kT
        replay()
    ctx.integrator.setTemperature(310.0)
    assert lib.calls["tgnh_set_temperatures"] == 1
    ctx.close()
