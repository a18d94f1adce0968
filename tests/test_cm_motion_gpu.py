"""GPU tests of tgnh_get_momentum, tgnh_remove_cm_motion, tgnh_shift_velocities and tgnh_set_cm_motion_removal
(tgnh_cm_motion.hip) against `momentum` / `removed` of tests/test_cm_motion.py: the header's formulas restated in numpy.

Velocities: the device draw from a fixed seed plus a drift of (0.3, -0.2, 0.1) nm/ps on every massive slot -- v_cm far from zero --,
read back once per system and precision and handed to every handle under comparison.

Tolerances, all formulas.  `massive` is exact.  The per-slot terms (m; m vx, m vy, m vz) are the same fp64 operations on both sides,
each rounded on its own, and only the order of the n additions differs; a sum of n terms in any order lies within
(n - 1) 2^-53 sum|term| (1 + O(n 2^-53)) of the exact sum, so two orders differ by less than n 2^-52 sum|term|: dM and dP below.
v_cm = P / M then differs by at most (dP + |v_cm| dM) / M (first order in the two; the division's own rounding and the second
order are a part in 10^16 of that, and the sums themselves sit a factor sqrt(n) inside their bounds).  A velocity after removal: that
bound, plus one unit in the last place of velm's type at the yardstick's value (the one rounding of the store, taken at a value
that may sit on the other side of a rounding boundary).  The momentum left, summed by the yardstick: every stored v' is off by at
most u |v'| (u = 2^-53 for double4, 2^-24 for float4) -- sum m u |v'| --, M times the error of v_cm is at most dP + |v_cm| dM, and the
yardstick's own sum of the result is covered by the same two (sum|m v'| <= sum|m v| + |v_cm| sum m).  w of every slot and every
component of a massless slot: bit for bit.

DEFER_SCALE.  Between two steps of such a handle tgnh_state_changed is refused, and tgnh_flush does not take back the thermostat
half that has already run: it stays refused after the flush (tests/test_velocity_init_gpu.py has the same for the velocity draw).
The remover and the shift answer what tgnh_state_changed answers, before and after the flush, with velm untouched where that is
a refusal; where tgnh_state_changed is accepted -- the same handle before its first step, a handle without the flag after a flush
-- they work."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import (DrudeTGNHIntegrator, HipContext, TgnhError, FLAG_DEFER_SCALE, FLAG_WAVE_TILES,
                                                   FLAG_TRUST_STATE_CHANGED, FLAG_GATHER)
from test_cm_motion import momentum, removed, shifted, new_momentum, STORE

pytestmark = pytest.mark.gpu

DRIFT = (0.3, -0.2, 0.1)
SEED = 20241018
PRECISIONS = ("double", "mixed", "single")


def _drudes_at_the_end():
    from helpers import drudes_at_the_end                  # (the builder behind test_drude_stats.gpu_cases()' gather case)
    return drudes_at_the_end(300)


# the smallest shapes at which each stage can go wrong: 5 slots per water, one of them massless; work-groups of 256
SYSTEMS = {"water1": lambda: synth.water_box(1),            # 5 slots: part of one wavefront
           "water13": lambda: synth.water_box(13),          # 65: into a second wavefront
           "water52": lambda: synth.water_box(52),          # 260: a second work-group holding four slots
           "water52430": lambda: synth.water_box(52_430),   # 262 150: six slots beyond 1024 x 256 -- the grid cap, a second trip of the grid-stride loop
           "nacl": synth.nacl,                              # 2 500: unequal masses
           "drudes-at-the-end": _drudes_at_the_end}         # the gather path
_cache = {}


def system(name):
    if name not in _cache:
        _cache[name] = SYSTEMS[name]()[0]
    return _cache[name]


def integ(chains=3):
    return DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, chains, True, True)


def context(s, precision="mixed", flags=0, mode="TGNH", **kw):
    return HipContext(s, integ(), mode=mode, precision=precision, flags=flags, **kw)


def read(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    return ctx.velm.cpu().numpy()


def load(ctx, velm):
    """these velocities into the context's velm, as a setVelocities"""
    ctx._state_changed()
    ctx.velm.copy_(ctx.torch.from_numpy(np.ascontiguousarray(velm)).to(ctx.dev))


def drawn(name, precision):
    """velm [N, 4] of the case in its stored type: drawn on the device, drifted, read back; built once and never changed"""
    key = (name, precision, "velm")
    if key not in _cache:
        ctx = context(system(name), precision)
        ctx.setVelocitiesToTemperature(300.0, SEED, 1.0)
        massive = ctx.velm[:, 3] != 0
        ctx.velm[massive, :3] += ctx.torch.tensor(DRIFT, dtype=ctx.mdt, device=ctx.dev)
        velm = read(ctx)
        ctx.close()
        assert velm.dtype == STORE[precision]
        velm.setflags(write=False)
        _cache[key] = velm
    return _cache[key]


def reference(name, precision):
    key = (name, precision, "ref")
    if key not in _cache:
        velm = drawn(name, precision)
        _cache[key] = (momentum(velm, precision), removed(velm, precision))
    return _cache[key]


def bounds(ref):
    """dM, dP [3] and the bound on v_cm [3] that follows from the two"""
    dM = ref.massive * 2.0 ** -52 * ref.abs_mass
    dP = ref.massive * 2.0 ** -52 * ref.abs_momentum
    return dM, dP, (dP + np.abs(ref.velocity) * dM) / ref.mass


def raw(ctx):
    st = new_momentum()
    rc = ctx.lib.tgnh_get_momentum(ctx.h, ctx._stream(), C.byref(st))
    assert rc == _lib.TGNH_OK, ctx.lib.tgnh_last_error()
    return bytes(st)


def check_removed(out, velm, want, ref, precision, what):
    """out: velm after the removal; velm: before; want: the yardstick's result; ref: the yardstick's sums of velm"""
    dM, dP, dV = bounds(ref)
    massless = ~ref.mask
    assert out[:, 3].tobytes() == velm[:, 3].tobytes()                              # w of every slot
    assert out[massless].tobytes() == velm[massless].tobytes()                      # every component of a massless slot
    err = np.abs(out[ref.mask, :3].astype(np.float64) - want[ref.mask, :3].astype(np.float64))
    ulp = np.spacing(np.abs(want[ref.mask, :3])).astype(np.float64)                 # (of velm's type)
    left = momentum(out, precision)
    u = 2.0 ** -24 if precision == "single" else 2.0 ** -53
    allowed = u * left.abs_momentum + dP + np.abs(ref.velocity) * dM
    print(f"{what}: max |dv'| / (bound + ulp) = {(err / (dV + ulp)).max():.3e}; momentum left {left.momentum} / allowed {allowed}")
    assert (err <= dV + ulp).all()
    assert (np.abs(left.momentum) <= allowed).all()


# ---- 1. exactness
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_against_the_header(name, precision):
    s = system(name)
    velm = drawn(name, precision)
    ref, want = reference(name, precision)
    assert ref.massive == int((s.mass > 0).sum()) < s.num_particles
    assert np.abs(ref.velocity).max() > 0.05                                        # (the drift: v_cm is far from zero)
    ctx = context(s, precision)
    assert ctx.step_path()[0] == ("gather" if name == "drudes-at-the-end" else "tiled")
    load(ctx, velm)
    got = ctx.momentum()
    dM, dP, dV = bounds(ref)
    eM, eP, eV = abs(got.mass - ref.mass), np.abs(got.momentum - ref.momentum), np.abs(got.velocity - ref.velocity)
    print(f"{name} {precision}: massive {got.massive} |dM| {eM:.3e} / {dM:.3e}  |dP| {eP} / {dP}  |dv_cm| {eV} / {dV}")
    assert got.massive == ref.massive
    assert eM <= dM and (eP <= dP).all() and (eV <= dV).all()
    assert ctx.momentum().raw == got.raw                                            # asked twice
    assert read(ctx).tobytes() == velm.tobytes()                                    # a query writes nothing
    ctx.removeCMMotion()
    assert ctx.pending_state() & (1 << 9) == 0
    check_removed(read(ctx), velm, want, ref, precision, f"{name} {precision}")
    ctx.close()


# ---- 2. one answer whatever the handle
@pytest.mark.parametrize("name", ["water52", "nacl"])
def test_one_answer_whatever_the_handle(name):
    s = system(name)
    velm = drawn(name, "mixed")
    want, paths = None, set()
    for mode, flags in (("TGNH", 0), ("TGNH", FLAG_GATHER), ("dualNH", 0), ("TGNH", FLAG_WAVE_TILES)):
        ctx = context(s, flags=flags, mode=mode)
        paths.add(ctx.step_path()[0])
        load(ctx, velm)
        a, b = raw(ctx), raw(ctx)
        assert a == b, (mode, flags)                                                # asked twice
        ctx.removeCMMotion()
        got = (a, read(ctx).tobytes())
        want = got if want is None else want
        assert got == want, (mode, flags)
        ctx.close()
    assert paths == {"tiled", "gather"}


# ---- 3. handle state
def state_bytes(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    out = [ctx.posq.cpu().numpy().tobytes(), ctx.velm.cpu().numpy().tobytes()]
    if ctx.posq_corr is not None:
        out.append(ctx.posq_corr.cpu().numpy().tobytes())
    return out + [ctx.thermostat_state(k).tobytes() for k in range(4)]


def test_the_remover_drops_carried_kinetic_energies():
    s = system("water52")
    velm = drawn("water52", "mixed")
    a, b = context(s, flags=FLAG_TRUST_STATE_CHANGED), context(s, flags=FLAG_TRUST_STATE_CHANGED)
    for ctx in (a, b):
        load(ctx, velm)
        ctx.step(1)
        assert ctx.pending_state() & (1 << 9)                                       # the next half would start from the carried sums
    assert state_bytes(a) == state_bytes(b)
    a.removeCMMotion()
    assert a.pending_state() & (1 << 9) == 0
    b.setVelocities(read(a)[:, :3])                                                 # (velm is fp64 in mixed precision: the same bits)
    assert b.pending_state() & (1 << 9) == 0
    for ctx in (a, b):
        ctx.step(1)
    assert state_bytes(a) == state_bytes(b)
    # the shift invalidates alike
    assert a.pending_state() & (1 << 9)
    a.shift_velocities([0.01, 0.0, -0.01])
    assert a.pending_state() & (1 << 9) == 0
    b.setVelocities(read(a)[:, :3])
    for ctx in (a, b):
        ctx.step(1)
    assert state_bytes(a) == state_bytes(b)
    a.close()
    b.close()


def test_inside_a_deferred_sequence():
    s = system("water52")
    velm = drawn("water52", "mixed")
    lib = _lib.load()
    dv = (C.c_double * 3)(0.01, 0.02, 0.03)
    ctx, plain = context(s, flags=FLAG_DEFER_SCALE), context(s)
    # nothing owed yet: tgnh_state_changed is accepted, and so are the two
    load(ctx, velm)
    assert lib.tgnh_remove_cm_motion(ctx.h, ctx._stream()) == _lib.TGNH_OK
    assert read(ctx).tobytes() == reference_bytes(plain, velm)
    assert lib.tgnh_shift_velocities(ctx.h, dv, ctx._stream()) == _lib.TGNH_OK
    for c in (ctx, plain):
        load(c, velm)
        c.step(3)
    before = read(ctx)
    refused = lib.tgnh_state_changed(ctx.h)
    assert refused == _lib.ERR_STATE
    assert lib.tgnh_remove_cm_motion(ctx.h, ctx._stream()) == refused
    assert lib.tgnh_shift_velocities(ctx.h, dv, ctx._stream()) == refused
    with pytest.raises(TgnhError):
        ctx.removeCMMotion()
    assert read(ctx).tobytes() == before.tobytes()
    # the query flushes by itself; after the flush it finds nothing to do and leaves the handle as it found it
    first = ctx.momentum()
    assert lib.tgnh_flush(ctx.h, ctx._stream()) == _lib.TGNH_OK
    flushed = read(ctx)
    assert flushed.tobytes() != before.tobytes()
    bits = ctx.pending_state()
    got = ctx.momentum()
    assert ctx.pending_state() == bits and got.raw == first.raw
    assert read(ctx).tobytes() == flushed.tobytes()
    # ... and answers what a handle of the plain structure answers after the same steps
    want = plain.momentum()
    ref = momentum(read(plain), "mixed")
    dM, dP, _ = bounds(ref)
    print(f"deferred vs plain: |dM| {abs(got.mass - want.mass):.3e} / {dM:.3e}  |dP| {np.abs(got.momentum - want.momentum)} / {dP}")
    assert got.massive == want.massive and abs(got.mass - want.mass) <= dM and (np.abs(got.momentum - want.momentum) <= dP).all()
    # after the flush: what tgnh_state_changed answers (see the head of this file), velm untouched where that is a refusal
    after = lib.tgnh_state_changed(ctx.h)
    assert lib.tgnh_remove_cm_motion(ctx.h, ctx._stream()) == after
    assert lib.tgnh_shift_velocities(ctx.h, dv, ctx._stream()) == after
    assert after == _lib.TGNH_OK or read(ctx).tobytes() == flushed.tobytes()
    # a handle without the flag, after a flush: they work
    assert lib.tgnh_flush(plain.h, plain._stream()) == _lib.TGNH_OK
    v0 = read(plain)
    plain.removeCMMotion()
    check_removed(read(plain), v0, removed(v0, "mixed"), ref, "mixed", "plain handle after three steps")
    assert lib.tgnh_shift_velocities(plain.h, dv, plain._stream()) == _lib.TGNH_OK
    # the setter: not on a deferred handle
    assert lib.tgnh_set_cm_motion_removal(ctx.h, 1) == _lib.ERR_UNSUPPORTED
    with pytest.raises(TgnhError):
        context(s, flags=FLAG_DEFER_SCALE, cm_motion_removal=1)
    ctx.close()
    plain.close()


def reference_bytes(ctx, velm):
    """velm after the removal on a handle of the plain structure"""
    load(ctx, velm)
    ctx.removeCMMotion()
    return read(ctx).tobytes()


def test_errors_on_a_live_handle():
    s = system("nacl")
    velm = drawn("nacl", "mixed")
    ctx = context(s)
    load(ctx, velm)
    lib = ctx.lib
    st = new_momentum()
    assert lib.tgnh_get_momentum(ctx.h, ctx._stream(), C.byref(st)) == _lib.TGNH_OK
    kept = bytes(st)
    bad = new_momentum(C.sizeof(st) - 8)
    assert lib.tgnh_get_momentum(ctx.h, ctx._stream(), C.byref(bad)) == _lib.ERR_ARG
    assert lib.tgnh_get_momentum(ctx.h, ctx._stream(), None) == _lib.ERR_ARG
    for k in range(3):
        dv = (C.c_double * 3)(0.0, 0.0, 0.0)
        dv[k] = np.nan
        assert lib.tgnh_shift_velocities(ctx.h, dv, ctx._stream()) == _lib.ERR_ARG
    assert lib.tgnh_shift_velocities(ctx.h, None, ctx._stream()) == _lib.ERR_ARG
    assert lib.tgnh_set_cm_motion_removal(ctx.h, -1) == _lib.ERR_ARG
    with pytest.raises(TgnhError):
        ctx.shift_velocities([0.0, 1.0])
    assert read(ctx).tobytes() == velm.tobytes() and raw(ctx) == kept
    # an explicit shift is the header's formula too
    ctx.shift_velocities(DRIFT)
    assert read(ctx).tobytes() == shifted(velm, "mixed", DRIFT).tobytes()
    # the mailboxes cannot be attached while removal is on
    ctx.set_cm_motion_removal(2)
    _, ptr = ctx.exchange_create(1, 0)
    with pytest.raises(TgnhError) as e:
        ctx.exchange_attach_pointers([ptr])
    assert e.value.status == _lib.ERR_UNSUPPORTED
    ctx.set_cm_motion_removal(0)
    ctx.exchange_attach_pointers([ptr])
    with pytest.raises(TgnhError) as e:
        ctx.set_cm_motion_removal(2)
    assert e.value.status == _lib.ERR_UNSUPPORTED
    ctx.exchange_detach()
    ctx.close()


def test_the_draw_with_the_momentum_taken_off():
    s = system("nacl")
    a, b = context(s), context(s)
    a.setVelocitiesToTemperature(300.0, 11, 1.0, removeCMMotion=True)
    b.setVelocitiesToTemperature(300.0, 11, 1.0)
    v0 = read(b)
    ref = momentum(v0, "mixed")
    assert (np.abs(ref.momentum) > 1e-3 * ref.abs_momentum / np.sqrt(ref.massive)).any()       # (the draw leaves a net momentum)
    b.removeCMMotion()
    assert read(a).tobytes() == read(b).tobytes()
    check_removed(read(a), v0, removed(v0, "mixed"), ref, "mixed", "draw + removal")
    a.close()
    b.close()


# ---- 4. in the loop
@pytest.mark.parametrize("every", [1, 3])
def test_removal_inside_the_step_loop(every):
    s = system("water52")
    velm = drawn("water52", "double")
    a, b = context(s, "double", cm_motion_removal=every), context(s, "double")
    for ctx in (a, b):
        load(ctx, velm)

    def follow(upto):
        """the twin, a step at a time, the remover called by hand before the steps whose number is a multiple of `every`"""
        k = b.time()[1]
        while k < upto:
            if k % every == 0:
                b.removeCMMotion()
            b.step(1)
            k += 1

    a.step(7)
    follow(7)
    assert a.time() == b.time() and state_bytes(a) == state_bytes(b)
    assert state_bytes(a)[1] != velm.tobytes()
    # a recording bakes its removals in: only multiples of the interval, from a multiple
    if every == 3:
        for steps in (3, 2):                                 # the step count is 7; at 9, two steps are no multiple
            with pytest.raises(TgnhError) as e:
                a.capture_steps(steps)
            assert e.value.status == _lib.ERR_STATE
            a.step(2)
        assert a.time()[1] == 11
        a.step(1)
    else:
        a.step(5)
    assert a.time()[1] == 12
    replay = a.capture_steps(3)
    replay()
    replay()
    a.torch.cuda.synchronize(a.dev)
    assert a.time()[1] >= 18
    follow(a.time()[1])
    assert a.time() == pytest.approx(b.time(), rel=1e-12) and state_bytes(a) == state_bytes(b)
    a.close()
    b.close()


# ---- 5. sharded, on one GPU
@pytest.mark.parametrize("precision", ["mixed", "single"])
def test_two_shards_remove_one_momentum(precision):
    s = system("water52")
    velm = drawn("water52", precision)
    ref, want = reference("water52", precision)
    cut = 5 * 26                                             # cut at a molecule: slot 130, not a multiple of 64
    halves = [(0, cut), (cut, s.num_particles)]
    ranks = [context(s.slice_molecules(lo, hi), precision) for lo, hi in halves]
    for ctx, (lo, hi) in zip(ranks, halves):
        load(ctx, velm[lo:hi])
    own = [ctx.momentum() for ctx in ranks]
    assert sum(m.massive for m in own) == ref.massive
    calls = []
    for k, ctx in enumerate(ranks):
        other = own[1 - k]
        add = ctx.torch.tensor([other.mass, *other.momentum], dtype=ctx.torch.float64, device=ctx.dev)

        def allreduce(t, add=add, k=k):
            assert t.numel() == 4
            calls.append(k)
            t += add
        ctx.set_allreduce(allreduce)
    for ctx in ranks:
        ctx.removeCMMotion()
    out = [read(ctx) for ctx in ranks]
    assert calls == [0, 1]
    check_removed(np.concatenate(out), velm, want, ref, precision, f"two shards {precision}")
    # both ranks used the same v_cm bits: the one the two ranks' sums give (a + b and b + a are the same fp64 number)
    M = own[0].mass + own[1].mass
    vcm = (own[0].momentum + own[1].momentum) / M
    for o, (lo, hi) in zip(out, halves):
        assert o.tobytes() == shifted(velm[lo:hi], precision, vcm).tobytes()
    for ctx in ranks:
        ctx.close()
    # mailboxes in place of the hook: no exchange for the momentum; the caller's route gives the same result
    ranks = [context(s.slice_molecules(lo, hi), precision) for lo, hi in halves]
    boxes = [ctx.exchange_create(2, k)[1] for k, ctx in enumerate(ranks)]
    for ctx, (lo, hi) in zip(ranks, halves):
        ctx.exchange_attach_pointers(boxes)
        load(ctx, velm[lo:hi])
        with pytest.raises(TgnhError) as e:
            ctx.removeCMMotion()
        assert e.value.status == _lib.ERR_UNSUPPORTED
        assert read(ctx).tobytes() == velm[lo:hi].tobytes()
    again = [ctx.momentum() for ctx in ranks]
    assert [m.raw for m in again] == [m.raw for m in own]
    for ctx in ranks:
        ctx.shift_velocities(vcm)
    for ctx, o in zip(ranks, out):
        assert read(ctx).tobytes() == o.tobytes()
    for ctx in ranks:
        ctx.exchange_detach()
    for ctx in ranks:
        ctx.close()
