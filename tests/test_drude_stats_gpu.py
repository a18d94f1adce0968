"""GPU tests of tgnh_get_drude_statistics (tgnh_drude_stats.hip) against `stats` of tests/test_drude_stats.py: the header's
formulas restated in numpy.

Tolerances.  pairs, over, hist and worst_particle are integers and compared exactly -- after `conditions` has asserted, on the
yardstick alone and over every pair, that no distance lies within a relative 1e-9 of the threshold or of a bin edge and that the
largest d2 is the largest alone (a few ulp of difference in a d cannot move a count then).  max_distance: 4 ulp.  sum_d2 and the
dipole components: the per-pair terms are the same fp64 operations on both sides, each rounded on its own, and only the order of
the P additions differs; a sum of P terms in any order lies within (P - 1) 2^-53 sum|term| (1 + O(P 2^-53)) of the exact sum, so
two orders differ by less than P 2^-52 sum|term| -- written below as that formula."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import (HipContext, TgnhError, create_handle, FLAG_DEFER_SCALE, FLAG_RESIDENT_STEP,
                                                   FLAG_WAVE_TILES, FLAG_GATHER)
from test_drude_stats import stats, configure, conditions, gpu_cases, integ, new_stats, THRESHOLD, HIST_MAX, BINS

pytestmark = pytest.mark.gpu

CASES = gpu_cases()
_cache = {}


def case(name):
    """(system, positions, charges) of a case, built once"""
    if name not in _cache:
        s = CASES[name][0]()[0]
        _cache[name] = (s,) + configure(s)
    return _cache[name]


def reference(name, precision, threshold=THRESHOLD, hist_max=HIST_MAX):
    key = (name, precision, threshold, hist_max)
    if key not in _cache:
        s, pos, q = case(name)
        _cache[key] = stats(s, pos, q, precision, threshold, hist_max)
    return _cache[key]


def context(s, pos, q, precision="mixed", flags=0, mode="TGNH", hardwall=0.0):
    ctx = HipContext(s, integ(hardwall), mode=mode, precision=precision, flags=flags)
    ctx.setPositions(pos)
    ctx.setCharges(q)
    return ctx


def raw(ctx, threshold=THRESHOLD, hist_max=HIST_MAX):
    st = new_stats()
    rc = ctx.lib.tgnh_get_drude_statistics(ctx.h, threshold, hist_max, ctx._stream(), C.byref(st))
    assert rc == _lib.TGNH_OK, ctx.lib.tgnh_last_error()
    return st


def sum_bound(P, abs_sum):
    return P * 2.0 ** -52 * abs_sum


def compare(got, ref, what, index_offset=0):
    """got: a DrudeStatistics, or a namespace with its fields; ref: the yardstick's"""
    P = ref.pairs
    err_d2 = abs(got.sum_d2 - ref.sum_d2)
    err_p = np.abs(np.asarray(got.induced_dipole) - ref.dipole)
    print(f"{what}: pairs {got.pairs} over {got.over} worst {got.worst_particle} max {got.max_distance!r} (ref {ref.max_distance!r}) "
          f"|sum_d2 err| {err_d2:.3e} / {sum_bound(P, ref.abs_sum_d2):.3e}  |dipole err| {err_p} / {sum_bound(P, ref.abs_dipole)}")
    assert got.pairs == ref.pairs and got.over == ref.over
    assert np.array_equal(got.hist, ref.hist)
    assert got.worst_particle + (index_offset if got.worst_particle >= 0 else 0) == ref.worst_particle
    assert abs(got.max_distance - ref.max_distance) <= 4 * np.spacing(ref.max_distance)
    assert err_d2 <= sum_bound(P, ref.abs_sum_d2)
    assert (err_p <= sum_bound(P, ref.abs_dipole)).all()


# ---- 1. exactness
@pytest.mark.parametrize("name,precision", [(n, p) for n, (_, precs) in CASES.items() for p in precs])
def test_against_the_header(name, precision):
    s, pos, q = case(name)
    ref = reference(name, precision)
    conditions(ref, THRESHOLD, HIST_MAX)                     # over every pair, on the yardstick alone
    assert ref.over > 0 and ref.hist[BINS] > 0
    ctx = context(s, pos, q, precision)
    assert ctx.step_path()[0] == ("gather" if name == "drudes-at-the-end" else "tiled")
    got = ctx.drude_statistics(THRESHOLD, HIST_MAX)
    compare(got, ref, f"{name} {precision}")
    assert got.rms_distance == np.sqrt(got.sum_d2 / got.pairs) and got.hist_edges[-1] == HIST_MAX
    # no histogram asked for: the rest stays what it is, bit for bit
    off = ctx.drude_statistics(THRESHOLD, 0.0)
    assert not off.hist.any() and off.hist_edges is None
    assert (off.pairs, off.over, off.worst_particle, off.max_distance, off.sum_d2) == (got.pairs, got.over, got.worst_particle, got.max_distance, got.sum_d2)
    assert off.induced_dipole.tobytes() == got.induced_dipole.tobytes()
    # only the Drude particles' charges enter
    q2 = q.copy()
    q2[np.setdiff1d(np.arange(s.num_particles), s.pair_drude)] += 1.5
    ctx.setCharges(q2)
    assert ctx.drude_statistics(THRESHOLD, HIST_MAX).raw == got.raw
    # threshold = None: the integrator's wall (0: every pair that is not exactly on its parent)
    assert ctx.drude_statistics().over == int((ref.d2 > 0).sum())
    ctx.close()


# ---- 2. one answer whatever the path
@pytest.mark.parametrize("name", ["nacl", "water216"])
def test_one_answer_whatever_the_path(name):
    s, pos, q = case(name)
    want, paths = None, set()
    for flags in (0, FLAG_WAVE_TILES, FLAG_DEFER_SCALE | FLAG_RESIDENT_STEP, FLAG_GATHER):
        ctx = context(s, pos, q, flags=flags)
        paths.add(ctx.step_path()[0])
        a, b = bytes(raw(ctx)), bytes(raw(ctx))
        assert a == b, flags                                 # asked twice
        want = a if want is None else want
        assert a == want, flags
        ctx.close()
    assert paths == {"tiled", "gather"}


# ---- 3. sharding
def test_shards_add_up():
    name = "water216"
    s, pos, q = case(name)
    ref = reference(name, "mixed")
    cut = 5 * 100                                            # molecule 100: slot 500, not a multiple of 64
    assert cut % 64 != 0
    parts = []
    for lo, hi in ((0, cut), (cut, s.num_particles)):
        ctx = context(s.slice_molecules(lo, hi), pos[lo:hi], q[lo:hi])
        parts.append((lo, ctx.drude_statistics(THRESHOLD, HIST_MAX)))
        ctx.close()
    assert all(p.pairs > 0 for _, p in parts)
    lo_w, worst = max(parts, key=lambda t: t[1].max_distance)
    from types import SimpleNamespace
    total = SimpleNamespace(pairs=sum(p.pairs for _, p in parts), over=sum(p.over for _, p in parts),
                            hist=sum(p.hist for _, p in parts), sum_d2=sum(p.sum_d2 for _, p in parts),
                            induced_dipole=sum(p.induced_dipole for _, p in parts),
                            max_distance=worst.max_distance, worst_particle=worst.worst_particle + lo_w)
    compare(total, ref, "two shards")


# ---- 4. a query is not a step
def state_bits(ctx):
    out = [ctx.pending_state()]
    ctx.flush()
    ctx.torch.cuda.synchronize(ctx.dev)
    out += [ctx.posq.cpu().numpy().tobytes(), ctx.posq_corr.cpu().numpy().tobytes(), ctx.velm.cpu().numpy().tobytes()]
    out += [ctx.thermostat_state(k).tobytes() for k in range(4)]
    out.append(ctx.pending_state())
    return out


@pytest.mark.parametrize("flags", [FLAG_DEFER_SCALE | FLAG_RESIDENT_STEP, 0])
def test_a_query_is_not_a_step(flags):
    s, pos, q = case("water216")
    asked, twin = context(s, pos, q, flags=flags), context(s, pos, q, flags=flags)
    for ctx in (asked, twin):
        ctx.compute_forces()
    seen = []
    for _ in range(20):
        for ctx in (asked, twin):
            ctx.step_begin()
            ctx.compute_forces()
            ctx.step_end()
        before = asked.pending_state()
        seen.append(asked.drude_statistics(THRESHOLD, HIST_MAX).max_distance)
        assert asked.pending_state() == before
    assert len(set(seen)) > 1                                # (the answers follow the trajectory)
    assert state_bits(asked) == state_bits(twin)
    assert asked.check() == 0 and twin.check() == 0
    asked.close()
    twin.close()


# ---- 5. it sees what the step does
def test_it_sees_the_hard_wall():
    s, _, q = case("water216")
    pos = np.array(s.positions, np.float64)                  # (the builder's own start: every Drude particle within 0.001 nm of its parent)
    out = [3, 77, 215]                                       # pairs started at 0.03 nm: beyond the wall, below twice the wall
    pos[s.pair_drude[out]] = pos[s.pair_parent[out]] + [0.03, 0.0, 0.0]
    vel = np.array(s.velocities, np.float64)                 # ... and on their way out, as a Drude particle beyond the wall is: the wall
    vel[s.pair_drude[out]] = vel[s.pair_parent[out]] + [0.1, 0.0, 0.0]     # reverses the relative motion it finds (Ref :299-383)
    ctx = context(s, pos, q, hardwall=0.02)
    ctx.setVelocities(vel)
    ctx.force.zero_()                                        # (no spring pulls them back before the wall does)
    got = ctx.drude_statistics()                             # threshold: the integrator's wall
    assert got.threshold == 0.02 and got.over == len(out) and abs(got.max_distance - 0.03) < 1e-6
    ctx.step_begin()
    after = ctx.drude_statistics()
    print(f"after step_begin: over {after.over}, max {after.max_distance!r}")
    assert after.over == 0 and after.pairs == s.num_pairs
    assert ctx.status_flags() & 1 == 0
    ctx.close()


# ---- 6. errors on a live handle
def test_errors_on_a_live_handle():
    s, pos, q = case("nacl")
    ctx = context(s, pos, q)
    call = ctx.lib.tgnh_get_drude_statistics
    st = raw(ctx)
    before = bytes(st)
    for thr, hmax in ((-1.0, 0.0), (np.nan, 0.0), (np.inf, 0.01), (0.02, -0.01), (0.02, np.nan), (0.02, np.inf)):
        assert call(ctx.h, thr, hmax, ctx._stream(), C.byref(st)) == _lib.ERR_ARG, (thr, hmax)
    assert bytes(st) == before                               # *out untouched
    bad = new_stats(C.sizeof(st) - 8)
    kept = bytes(bad)
    assert call(ctx.h, 0.02, 0.0, ctx._stream(), C.byref(bad)) == _lib.ERR_ARG and bytes(bad) == kept
    assert call(ctx.h, 0.02, 0.0, ctx._stream(), None) == _lib.ERR_ARG
    assert call(None, 0.02, 0.0, ctx._stream(), C.byref(st)) == _lib.ERR_ARG
    with pytest.raises(TgnhError):
        ctx.drude_statistics(-1.0)
    # buffers not bound
    it = integ()
    group, ngroups = it._resolve_groups(s.num_particles)
    h = create_handle(ctx.lib, s, it, group, ngroups, _lib.MODE_TGNH, _lib.PREC_MIXED, 0, 0, synth.KB, ctx.padded)
    assert call(h, 0.02, 0.0, ctx._stream(), C.byref(st)) == _lib.ERR_STATE
    assert bytes(st) == before
    assert ctx.lib.tgnh_destroy(h) == _lib.TGNH_OK
    ctx.close()


def test_a_handle_without_pairs():
    s = synth.DrudeSystem(mass=np.array([12.0, 1.0, 0.0]), pair_drude=np.zeros(0, np.int32), pair_parent=np.zeros(0, np.int32),
                          resid=np.zeros(3, np.int32), positions=np.arange(9.0).reshape(3, 3), velocities=np.zeros((3, 3)))
    ctx = context(s, s.positions, np.ones(3))
    got = ctx.drude_statistics(0.02, 0.05)
    assert (got.pairs, got.over, got.worst_particle, got.max_distance, got.sum_d2, got.rms_distance) == (0, 0, -1, 0.0, 0.0, 0.0)
    assert not got.hist.any() and not got.induced_dipole.any()
    ctx.close()
