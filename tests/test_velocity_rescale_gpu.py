"""GPU tests of tgnh_scale_velocities, tgnh_rescale_to_temperature, tgnh_get_rescale_factors and tgnh_set_velocity_rescaling
against the CPU oracle's scale_velocities / kinetic_energies (tests/test_velocity_rescale.py has the systems, the integrator, the
factor rule restated in numpy, and why two of the systems are never asked for their targets).

Velocities: the device draw at 300 K / 1 K from a fixed seed, read back once per system and precision and handed to every handle
under comparison.

Gates, none of them fitted to what the kernels give.
 1  velocities against the oracle: max-norm error relative to the larger of the largest input and the largest output speed, at most
    16 eps of velm's element type (3.6e-15 double and mixed, 1.9e-6 single): a count of roundings -- the pair form of the rescale
    puts about ten rounded operations between load and store, each on a term no larger than that speed.  Massless slots and every
    w: bit for bit.
 2  factors of different handles over the same velocities: 1e-12 relative, the header's figure for kinetic-energy sums added in
    different orders.
 3  kinetic energies after tgnh_rescale_to_temperature against N kT: 1e-12 relative in double and mixed; 16 x 2^-24 in single
    (stored fp32 velocities: eight roundings per component, doubled by the square).  Factors against numpy's sqrt(target / KE) of
    the sums read back: 1 ulp (the division is exact to rounding, HIP documents 1 ulp for its fp64 square root).
 Two scalings in a row (test 4): the first one's error is multiplied by the second one's largest factor before the second adds its
 own, so gate 1 is taken once at the intermediate speed times that factor and once at the final speed."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import _lib
from openmm_drudenose_amd.drudetgnhplugin import (HipContext, TgnhError, FLAG_DEFER_SCALE, FLAG_WAVE_TILES, FLAG_RESIDENT_STEP,
                                                   FLAG_TRUST_STATE_CHANGED, FLAG_GATHER)
from helpers import make_oracle
from test_cm_motion import momentum
from test_velocity_rescale import (SYSTEMS, ORACLE_ONLY, MODES, T_NEW, TD_NEW, KE_GATE, system, integ, to_oracle, targets,
                                   factor_rule, landing_com, plain_integrator)

pytestmark = pytest.mark.gpu

SEED = 20241019
PRECISIONS = ("double", "mixed", "single")
STORE = {"double": np.float64, "mixed": np.float64, "single": np.float32}
# what each system is for (the smallest shapes at which a stage can go wrong)
#   water1             5 slots: part of a wavefront, one of them massless
#   water13            65 slots: into a second wavefront
#   water300           1500 slots: several tiles and work-groups
#   nacl               unequal masses, two-slot ions
#   ionic4             two groups, 35-slot molecules
#   polymer            a 900-slot molecule: longer than a 512-slot tile -- the centre-of-mass table
#   groups40           42 thermostats: the gather path's own chain form
#   drudes-at-the-end  the gather path by topology
#   water52            260 slots: the handle-state, step-loop and sharding tests
#   spanning           a molecule in two groups: against the oracle only
TILE_SLOTS = 512
_cache = {}


def context(name, mode="TGNH", precision="mixed", flags=0, com=True, **kw):
    it, _, _ = integ(name, mode, com=com)
    return HipContext(system(name)[0], it, mode=mode, precision=precision, flags=flags, **kw)


def oracle(name, mode, com=True):
    it, g, ng = integ(name, mode, com=com)
    return make_oracle(system(name)[0], g, ng, mode, it)


def step_path_code(ctx):
    g = C.c_int()
    assert ctx.lib.tgnh_get_step_path(ctx.h, C.byref(g), None) == _lib.TGNH_OK
    return g.value


def read(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    return ctx.velm.cpu().numpy()


def load(ctx, velm):
    """these velocities into the context's velm, as a setVelocities"""
    ctx._state_changed()
    ctx.velm.copy_(ctx.torch.from_numpy(np.array(velm)).to(ctx.dev))                # (a copy: the cached array is read-only)


def drawn(name, precision):
    """velm [N, 4] of the case in its stored type: drawn on the device, read back; built once and never changed"""
    key = (name, precision)
    if key not in _cache:
        ctx = context(name, precision=precision)
        ctx.setVelocitiesToTemperature(300.0, SEED, 1.0)
        velm = read(ctx)
        ctx.close()
        assert velm.dtype == STORE[precision]
        velm.setflags(write=False)
        _cache[key] = velm
    return _cache[key]


def speed(v):
    return float(np.abs(np.asarray(v, np.float64)[:, :3]).max())


def eps(precision):
    return float(np.finfo(STORE[precision]).eps)


def check_velocities(out, velm, want, precision, what, scale=None):
    """gate 1.  out: velm after the call; velm: before; want [N, 3] fp64: the yardstick's velocities"""
    massless = velm[:, 3] == 0
    assert out[:, 3].tobytes() == velm[:, 3].tobytes()                              # w of every slot
    assert out[massless].tobytes() == velm[massless].tobytes()                      # every component of a massless slot
    err = float(np.abs(out[:, :3].astype(np.float64) - want).max())
    scale = max(speed(velm), speed(want)) if scale is None else scale
    print(f"{what}: max |dv| / speed = {err / scale:.3e} (gate {16 * eps(precision):.3e})")
    assert err <= 16 * eps(precision) * scale
    return err / scale


def fixed_factors(NT, mode, lo=0.5, hi=2.0):
    f = np.linspace(lo, hi, NT)
    if mode == "dualNH":
        f[1] = np.nan                                                               # the unused entry: not looked at
    return f


def oracle_scaled(o, velm, f, mode):
    v = np.ascontiguousarray(velm[:, :3], np.float64)
    o.scale_velocities(v, to_oracle(f, mode))
    return v


def nkt_at(ctx, temperature, drude_temperature):
    return targets(ctx.dof()[0], temperature, drude_temperature)


# ---- 1. against the oracle
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [n for n in SYSTEMS if n != "water52"])
def test_fixed_factors_against_the_oracle(name, mode, precision):
    velm = drawn(name, precision)
    for com in ((True, False) if name == "drudes-at-the-end" else (True,)):
        ctx = context(name, mode, precision, com=com)
        if name == "polymer" and mode == "TGNH":                                        # (dualNH keeps no residues)
            assert ctx.topology(5).max() > TILE_SLOTS and ctx.step_path()[0] == "tiled"   # (the handle's residue sizes) a molecule longer than a tile
        if name == "groups40":
            assert step_path_code(ctx) == (2 if mode == "TGNH" else 0)                  # the gather path's own chain form
            assert ctx.num_thermostats() == (42 if mode == "TGNH" else 3)
        if name == "drudes-at-the-end":
            assert ctx.step_path()[0] == "gather"
        f = fixed_factors(ctx.num_thermostats(), mode)
        want = oracle_scaled(oracle(name, mode, com), velm, f, mode)
        load(ctx, velm)
        bits = ctx.pending_state()
        ctx.scale_velocities(f)
        assert ctx.pending_state() == bits
        check_velocities(read(ctx), velm, want, precision, f"{name} {mode} {precision} com={com}")
        got = ctx.rescale_factors()
        live = ~np.isnan(f)
        assert np.array_equal(got[live], f[live]) and (got[~live] == 1.0).all()
        ctx.close()


# ---- 2. one answer whatever the handle
@pytest.mark.parametrize("name", ["water52", "nacl"])
def test_one_answer_whatever_the_handle(name):
    velm = drawn(name, "mixed")
    first, paths = None, set()
    for flags in (0, FLAG_WAVE_TILES, FLAG_RESIDENT_STEP, FLAG_GATHER, FLAG_TRUST_STATE_CHANGED):
        ctx = context(name, flags=flags)
        paths.add(ctx.step_path()[0])
        runs = []
        for _ in range(2):                                                          # asked twice from the same velocities
            load(ctx, velm)
            ctx.rescale_to_temperature(T_NEW, TD_NEW)
            runs.append((ctx.rescale_factors().tobytes(), read(ctx).tobytes()))
        assert runs[0] == runs[1], flags
        f, out = ctx.rescale_factors(), read(ctx)
        if first is None:
            first = (f, out)
        rel = np.abs(f - first[0]) / first[0]
        print(f"{name} flags {flags}: factors {f}, rel. difference to flags 0 {rel.max():.3e}")
        assert rel.max() <= 1e-12
        check_velocities(out, velm, first[1][:, :3].astype(np.float64), "mixed", f"{name} flags {flags} vs flags 0")
        ctx.close()
    assert paths == {"tiled", "gather"}


# ---- 3. landing on the targets
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [n for n in SYSTEMS if n not in ORACLE_ONLY])
def test_landing_on_the_targets(name, mode, precision):
    velm = drawn(name, precision)
    ctx = context(name, mode, precision, com=landing_com(name))
    load(ctx, velm)
    chain_factors = ctx.last_scale_factors()
    baths = ctx.dof()[1].copy()
    dof = ctx.dof()[0]
    want = nkt_at(ctx, T_NEW, TD_NEW)
    inert = dof == 0
    assert inert[1] if mode == "dualNH" else True
    ctx.rescale_to_temperature(T_NEW, TD_NEW)
    f, before = ctx.rescale_factors(), ctx.last_kinetic_energies()
    # the factors: the rule, of the sums as they were
    ref, nan = factor_rule(before, want, inert)
    assert not nan and (f[inert] == 1.0).all()
    ulps = np.abs(f - ref) / np.spacing(ref)
    print(f"{name} {mode} {precision}: factors {f[~inert].min():.4f} .. {f[~inert].max():.4f}, off numpy's by {ulps.max():.1f} ulp at the most")
    assert ulps.max() <= 1.0
    # the kinetic energies afterwards
    after = ctx.compute_kinetic_energies()
    live = want > 0
    miss = np.abs(after[live] - want[live]) / want[live]
    print(f"{name} {mode} {precision}: max rel. miss of N kT {miss.max():.3e} (gate {KE_GATE[precision]:.3e})")
    assert miss.max() <= KE_GATE[precision]
    # the baths and the chain's own factors are whose they were
    assert np.array_equal(ctx.dof()[1], baths) and np.array_equal(ctx.last_scale_factors(), chain_factors)
    assert ctx.status_flags() == 0
    # a temperature of zero: exact zeros on massive slots, the rest bit for bit
    ctx.rescale_to_temperature(0.0, 0.0)
    out = read(ctx)
    massive = velm[:, 3] != 0
    assert not out[massive, :3].any()
    assert out[:, 3].tobytes() == velm[:, 3].tobytes() and out[~massive].tobytes() == velm[~massive].tobytes()
    assert (ctx.rescale_factors()[~inert] == 0.0).all() and (ctx.rescale_factors()[inert] == 1.0).all()
    # ... and no kinetic energy left to scale: every factor is 1
    ctx.rescale_to_temperature(T_NEW, TD_NEW)
    assert (ctx.rescale_factors() == 1.0).all()
    ctx.close()


# ---- 4. back-to-back calls
@pytest.mark.parametrize("name", ["nacl", "groups40"])
def test_two_calls_in_a_row_each_apply_their_own_factors(name):
    velm = drawn(name, "mixed")
    ctx = context(name)
    NT = ctx.num_thermostats()
    f1, f2 = fixed_factors(NT, "TGNH"), fixed_factors(NT, "TGNH", 1.75, 0.25)
    o = oracle(name, "TGNH")
    mid = oracle_scaled(o, velm, f1, "TGNH")
    want = mid.copy()
    o.scale_velocities(want, f2)
    load(ctx, velm)
    buf = (C.c_double * NT)(*f1)                              # ONE array, rewritten while the first call is still queued
    ctx.torch.cuda.synchronize(ctx.dev)
    assert ctx.lib.tgnh_scale_velocities(ctx.h, buf, NT, ctx._stream()) == _lib.TGNH_OK
    buf[:] = list(f2)
    assert ctx.lib.tgnh_scale_velocities(ctx.h, buf, NT, ctx._stream()) == _lib.TGNH_OK
    buf[:] = [0.0] * NT
    scale = max(speed(velm), speed(mid)) * max(1.0, f2.max()) + max(speed(mid), speed(want))
    check_velocities(read(ctx), velm, want, "mixed", f"{name}: two scalings", scale=scale)
    assert np.array_equal(ctx.rescale_factors(), f2)
    ctx.close()


# ---- 5. handle state
def state_bytes(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    out = [ctx.posq.cpu().numpy().tobytes(), ctx.velm.cpu().numpy().tobytes()]
    if ctx.posq_corr is not None:
        out.append(ctx.posq_corr.cpu().numpy().tobytes())
    return out + [ctx.thermostat_state(k).tobytes() for k in range(4)]


def test_either_call_drops_carried_kinetic_energies():
    velm = drawn("water52", "mixed")
    a, b = context("water52", flags=FLAG_TRUST_STATE_CHANGED), context("water52", flags=FLAG_TRUST_STATE_CHANGED)
    for ctx in (a, b):
        load(ctx, velm)
        ctx.step(1)
    calls = (lambda: a.rescale_to_temperature(T_NEW, TD_NEW), lambda: a.scale_velocities(fixed_factors(a.num_thermostats(), "TGNH", 0.9, 1.1)))
    for call in calls:
        assert a.pending_state() & (1 << 9) and b.pending_state() & (1 << 9)       # the next half would start from the carried sums
        assert state_bytes(a) == state_bytes(b)
        chain_factors, bit8 = a.last_scale_factors(), a.pending_state() & (1 << 8)
        call()
        assert a.pending_state() & (1 << 9) == 0
        assert a.pending_state() & (1 << 8) == bit8
        assert np.array_equal(a.last_scale_factors(), chain_factors)
        assert state_bytes(a)[1] != state_bytes(b)[1]
        b.setVelocities(read(a)[:, :3])                                             # (velm is fp64 in mixed precision: the same bits)
        for ctx in (a, b):
            ctx.step(1)
        assert state_bytes(a) == state_bytes(b)
    a.close()
    b.close()


def test_inside_a_deferred_sequence():
    velm = drawn("water52", "mixed")
    lib = _lib.load()
    ctx, plain = context("water52", flags=FLAG_DEFER_SCALE), context("water52")
    NT = ctx.num_thermostats()
    f = (C.c_double * NT)(*fixed_factors(NT, "TGNH"))
    both = (lambda c: lib.tgnh_scale_velocities(c.h, f, NT, c._stream()), lambda c: lib.tgnh_rescale_to_temperature(c.h, T_NEW, TD_NEW, c._stream()))
    # nothing owed yet: tgnh_state_changed is accepted, and so are the two; the deferred handle gives what the plain one gives
    for call in both:
        outs = []
        for c in (ctx, plain):
            load(c, velm)
            assert call(c) == _lib.TGNH_OK
            outs.append(read(c))
        assert outs[0].tobytes() != velm.tobytes()
        check_velocities(outs[0], velm, outs[1][:, :3].astype(np.float64), "mixed", "deferred handle before its first step vs plain")
    for c in (ctx, plain):
        load(c, velm)
        c.step(2)
    before = read(ctx)
    kept = ctx.rescale_factors()
    assert lib.tgnh_state_changed(ctx.h) == _lib.ERR_STATE
    for call in both:
        assert call(ctx) == _lib.ERR_STATE
    with pytest.raises(TgnhError) as e:
        ctx.rescale_to_temperature()
    assert e.value.status == _lib.ERR_STATE
    with pytest.raises(TgnhError):
        ctx.scale_velocities(list(f))
    assert read(ctx).tobytes() == before.tobytes()
    assert np.array_equal(ctx.rescale_factors(), kept)
    # a handle without the flag, after a flush: they work
    assert lib.tgnh_flush(plain.h, plain._stream()) == _lib.TGNH_OK
    v0 = read(plain)
    chain_factors = plain.last_scale_factors()
    plain.rescale_to_temperature(T_NEW, TD_NEW)
    want = oracle_scaled(oracle("water52", "TGNH"), v0, plain.rescale_factors(), "TGNH")
    check_velocities(read(plain), v0, want, "mixed", "plain handle after two steps")
    assert np.array_equal(plain.last_scale_factors(), chain_factors)
    assert both[0](plain) == _lib.TGNH_OK
    # the setter: not on a deferred handle
    assert lib.tgnh_set_velocity_rescaling(ctx.h, 1, 300.0, 1.0) == _lib.ERR_UNSUPPORTED
    with pytest.raises(TgnhError) as e:
        ctx.set_velocity_rescaling(1)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    ctx.close()
    plain.close()


def test_errors_on_a_live_handle():
    velm = drawn("nacl", "mixed")
    ctx = context("nacl")
    lib, NT = ctx.lib, ctx.num_thermostats()
    load(ctx, velm)
    with pytest.raises(TgnhError) as e:
        ctx.rescale_factors()                                                       # nothing has been applied yet
    assert e.value.status == _lib.ERR_STATE
    for bad in ([1.0] * (NT - 1), [1.0] * (NT + 1), [1.0, -0.5, 1.0], [1.0, np.nan, 1.0], [np.inf, 1.0, 1.0], [[1.0, 1.0, 1.0]]):
        with pytest.raises(TgnhError) as e:
            ctx.scale_velocities(bad)
        assert e.value.status == _lib.ERR_ARG
    for t, td in ((-1.0, 1.0), (300.0, np.nan)):
        with pytest.raises(TgnhError) as e:
            ctx.rescale_to_temperature(t, td)
        assert e.value.status == _lib.ERR_ARG
    assert lib.tgnh_set_velocity_rescaling(ctx.h, -1, 300.0, 1.0) == _lib.ERR_ARG
    assert read(ctx).tobytes() == velm.tobytes()
    # the defaults are the integrator's temperatures
    ctx.rescale_to_temperature()
    after = ctx.compute_kinetic_energies()
    assert np.abs(after - ctx.dof()[1]).max() <= KE_GATE["mixed"] * ctx.dof()[1].max()
    # the mailboxes: no rescale to a temperature through them, none attached while rescaling is on; explicit factors pass
    ctx.set_velocity_rescaling(2)
    _, ptr = ctx.exchange_create(1, 0)
    with pytest.raises(TgnhError) as e:
        ctx.exchange_attach_pointers([ptr])
    assert e.value.status == _lib.ERR_UNSUPPORTED
    ctx.set_velocity_rescaling(0)
    ctx.exchange_attach_pointers([ptr])
    for call in (lambda: ctx.set_velocity_rescaling(2), lambda: ctx.rescale_to_temperature(T_NEW, TD_NEW)):
        kept = read(ctx).tobytes()
        with pytest.raises(TgnhError) as e:
            call()
        assert e.value.status == _lib.ERR_UNSUPPORTED and read(ctx).tobytes() == kept
    ctx.scale_velocities([1.0, 1.0, 1.0])
    ctx.exchange_detach()
    ctx.close()


# ---- 6. in the step loop
@pytest.mark.parametrize("with_removal", [False, True])
@pytest.mark.parametrize("every", [1, 3])
def test_rescaling_inside_the_step_loop(every, with_removal):
    velm = drawn("water52", "double")
    kw = {"cm_motion_removal": every} if with_removal else {}
    a, b = context("water52", precision="double", **kw), context("water52", precision="double")
    a.set_velocity_rescaling(every, T_NEW, TD_NEW)
    for ctx in (a, b):
        load(ctx, velm)
    for k in range(6):
        if k % every == 0:                                    # the twin, by hand: the removal first
            if with_removal:
                b.removeCMMotion()
            b.rescale_to_temperature(T_NEW, TD_NEW)
        b.step(1)
    a.step(6)
    assert a.time() == b.time() and state_bytes(a) == state_bytes(b)
    assert np.array_equal(a.rescale_factors(), b.rescale_factors())
    plain = context("water52", precision="double")
    load(plain, velm)
    plain.step(6)
    assert state_bytes(plain)[1] != state_bytes(a)[1]         # (the rescalings did change the trajectory)
    # switched off again, it is the plain loop
    a.set_velocity_rescaling(0)
    if with_removal:
        a.set_cm_motion_removal(0)
    b.setVelocities(read(a)[:, :3])
    a._state_changed()
    for ctx in (a, b):
        ctx.step(2)
    assert state_bytes(a) == state_bytes(b)
    for ctx in (a, b, plain):
        ctx.close()


def test_the_setter_is_refused_on_a_deferred_handle():
    ctx = context("water52", flags=FLAG_DEFER_SCALE)
    assert ctx.lib.tgnh_set_velocity_rescaling(ctx.h, 1, 300.0, 1.0) == _lib.ERR_UNSUPPORTED
    assert ctx.lib.tgnh_set_velocity_rescaling(ctx.h, 0, 300.0, 1.0) == _lib.TGNH_OK
    ctx.close()


# ---- 7. two shards on one GPU
@pytest.mark.parametrize("precision", ["mixed", "single"])
def test_two_shards_apply_one_set_of_factors(precision):
    s = system("water52")[0]
    velm = drawn("water52", precision)
    whole = context("water52", precision=precision)
    total = whole.local_dof_terms()
    load(whole, velm)
    whole.rescale_to_temperature(T_NEW, TD_NEW)
    cut = 5 * 26                                             # cut at a molecule: slot 130, not a multiple of 64
    halves = [(0, cut), (cut, s.num_particles)]
    ranks = [HipContext(s.slice_molecules(lo, hi), plain_integrator(), mode="TGNH", precision=precision, global_dof_sum=lambda local: total)
             for lo, hi in halves]                            # (one group: a shard's integrator needs no particle list)
    NT = whole.num_thermostats()
    for ctx, (lo, hi) in zip(ranks, halves):
        assert np.array_equal(ctx.dof()[0], whole.dof()[0])                         # the global degrees of freedom
        load(ctx, velm[lo:hi])
    assert np.allclose(sum(ctx.local_dof_terms() for ctx in ranks), total, rtol=1e-14)
    own = [ctx.compute_kinetic_energies() for ctx in ranks]                         # each rank's own sums first
    calls = []
    for k, ctx in enumerate(ranks):
        add = ctx.torch.tensor(own[1 - k], dtype=ctx.torch.float64, device=ctx.dev)

        def allreduce(t, add=add, k=k):
            assert t.numel() == NT
            calls.append(k)
            t += add
        ctx.set_allreduce(allreduce)
    for ctx in ranks:
        ctx.rescale_to_temperature(T_NEW, TD_NEW)
    out = [read(ctx) for ctx in ranks]
    assert calls == [0, 1]                                                          # once per rank, with NT values
    f = [ctx.rescale_factors() for ctx in ranks]
    assert f[0].tobytes() == f[1].tobytes()                                         # (a + b and b + a are the same fp64 number)
    for ctx in ranks:
        assert np.array_equal(ctx.last_kinetic_energies(), own[0] + own[1])
    rel = np.abs(f[0] - whole.rescale_factors()) / whole.rescale_factors()
    print(f"two shards {precision}: factors {f[0]}, rel. difference to the whole system's {rel.max():.3e}")
    assert rel.max() <= 1e-12
    check_velocities(np.concatenate(out), velm, read(whole)[:, :3].astype(np.float64), precision, f"two shards {precision}")
    for ctx in ranks + [whole]:
        ctx.close()


# ---- 8. an exact-temperature start
def test_the_draw_at_the_exact_temperature():
    a, b = context("nacl"), context("nacl")
    a.setVelocitiesToTemperature(300.0, 11, exact=True, removeCMMotion=True)
    b.setVelocitiesToTemperature(300.0, 11)
    v0 = read(b)
    b.removeCMMotion()
    b.rescale_to_temperature(300.0, 1.0)
    assert read(a).tobytes() == read(b).tobytes()                                   # the rescale runs last, after the removal
    # the momentum: within the remover's own bound (tests/test_cm_motion_gpu.py, check_removed) -- the rescale multiplies every
    # molecule's centre-of-mass velocity by ONE factor, so it scales the momentum the remover left and adds its roundings
    ref = momentum(v0, "mixed")
    dM = ref.massive * 2.0 ** -52 * ref.abs_mass
    dP = ref.massive * 2.0 ** -52 * ref.abs_momentum
    left = momentum(read(a), "mixed")
    allowed = 2.0 ** -53 * left.abs_momentum + dP + np.abs(ref.velocity) * dM
    print(f"draw, removal, rescale: momentum left {left.momentum} / allowed {allowed}; factors {a.rescale_factors()}")
    assert (np.abs(left.momentum) <= allowed).all()
    # the kinetic energies: on the handle's own N kT
    ke, nkt = a.compute_kinetic_energies(), a.dof()[1]
    miss = np.abs(ke - nkt) / nkt
    print(f"draw, removal, rescale: rel. miss of N kT {miss}")
    assert miss.max() <= KE_GATE["mixed"]
    assert not a.ke_sum_valid
    a.close()
    b.close()
