"""GPU tests of tgnh_minimize_begin / _iterate / _end, tgnh_get_minimize_state and tgnh_run_harness_minimize (tgnh_minimize.hip)
against `fire_sums`, `fire_decide` and `fire_update` of tests/test_minimize.py: the header's iteration restated in numpy.

Inputs: test_minimize.displaced -- every slot that is no Drude particle N(0, 0.02 nm) off its tether site, every Drude particle
N(0, 0.003 nm) off its parent -- with GPU_FIRE's parameters (a dt_max beyond the Drude spring's stability limit: 14 iterations take
every branch of the decision; tests/test_minimize.py asserts that, and that every decision's |P| stands 1000 x clear of its
summation bound).  Charges and the w of posq_correction are set to recognisable values: they must come back bit for bit.

Tolerances.  Each iteration is restated from the DEVICE'S OWN force words and `work`, read back before the iteration: the per-slot
terms of the three sums are then the same fp64 operations on both sides, each rounded on its own, and only the order of the n
additions differs; two orders of adding n terms differ by less than n 2^-52 sum|term| (tests/test_cm_motion_gpu.py has the
argument).  `moving` is exact.  Everything behind the sums -- the decision applied to the device's sums, the update with the
decision's scalars -- is the same sequence of IEEE operations on the same operands: bit for bit, in every precision.

A NaN cannot be planted in a force word -- the words are 64-bit integers, and the sums of their squares stay far below fp64's
range -- so the blown-up run of test 5 is made through the one input that can hold one: an entry of `work`."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import (TgnhError, FIRE_DEFAULTS, minimize_desc, FLAG_DEFER_SCALE, FLAG_WAVE_TILES, FLAG_GATHER)
from test_cm_motion_gpu import SYSTEMS, system, context, state_bytes, PRECISIONS
from test_minimize import (fire_sums, fire_decide, fire_update, new_state, moving_mask, displaced, coords, gpu_trace, GPU_FIRE, GPU_ITERATIONS,
                           CONVERGES_AFTER, TWO32)

pytestmark = pytest.mark.gpu

PAR = dict(FIRE_DEFAULTS, **GPU_FIRE)
_start = {}


def start(name):
    if name not in _start:
        pos = displaced(system(name))
        pos.setflags(write=False)
        _start[name] = pos
    return _start[name]


def dress(ctx, pos, first=0):
    """the displaced positions, and charges and correction w that are no zeros (numbered from the whole system's slot `first`)"""
    ctx.setPositions(pos)
    ctx.setCharges(np.arange(first, first + ctx.n) % 7 - 3.0)
    if ctx.posq_corr is not None:
        ctx.posq_corr[:, 3] = ctx.torch.arange(first, first + ctx.n, device=ctx.dev, dtype=ctx.torch.float32) % 5 + 1


def prepared(name, precision="mixed", **kw):
    """a context of the case, dressed"""
    ctx = context(system(name), precision, **kw)
    dress(ctx, start(name))
    return ctx


def stored(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    return ctx.posq.cpu().numpy(), None if ctx.posq_corr is None else ctx.posq_corr.cpu().numpy()


def words(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    return ctx.force.view(3, ctx.padded)[:, :ctx.n].cpu().numpy()


def work(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    return ctx.minimize_work.cpu().numpy()


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and (a[1] is None) == (b[1] is None) and (a[1] is None or a[1].tobytes() == b[1].tobytes())


def everything(ctx):
    """positions, the minimiser's velocity and the state block, as bytes"""
    p = stored(ctx)
    return [p[0].tobytes(), b"" if p[1] is None else p[1].tobytes(), work(ctx).tobytes(), ctx.minimize_state().raw]


def bits(*values):
    return np.array(values, np.float64).tobytes()


def status_of(call):
    try:
        call()
    except TgnhError as e:
        return e.status
    return _lib.TGNH_OK


def follow(ctx, mask, iterations, st=None, par=PAR, tolerance=0.0, what=""):
    """`iterations` x {force call-out, one iteration}, every one held against the restatement; -> (state, branches)"""
    st = new_state(par) if st is None else st
    branches = []
    for k in range(iterations):
        ctx.compute_forces()
        before, w0, F = stored(ctx), work(ctx), words(ctx)
        ctx.minimize_iterate()
        got = ctx.minimize_state()
        sums = fire_sums(F, w0, mask)
        eps = sums.n * 2.0 ** -52
        err = (abs(got.power - sums.P), abs(got.ff - sums.FF), abs(got.vv - sums.VV))
        allowed = (eps * sums.abs_P, eps * sums.abs_FF, eps * sums.abs_VV)
        print(f"{what} iteration {k}: |dP| {err[0]:.3e} / {allowed[0]:.3e}  |dFF| {err[1]:.3e} / {allowed[1]:.3e}  |dVV| {err[2]:.3e} / {allowed[2]:.3e}")
        assert got.moving == sums.n and all(e <= a for e, a in zip(err, allowed)), (k, err, allowed)
        st, branch = fire_decide(st, got.power, got.ff, got.vv, float(got.moving), par, tolerance)      # the device's sums
        branches.append(branch)
        assert bits(got.dt, got.alpha, got.rms_force) == bits(st.dt, st.alpha, st.rms_force), (k, branch)
        assert (got.iterations, got.uphill, got.since_uphill, got.converged) == (st.iterations, st.uphill, st.since_uphill, st.converged), (k, branch)
        want, wwork, _ = fire_update(before, w0, F, mask, st, par)
        assert same(stored(ctx), want), (k, branch)                                 # hi, lo, every w; a slot that does not move: byte for byte
        assert work(ctx).tobytes() == wwork.tobytes(), (k, branch)
    return st, branches


# ---- 1. each iteration against the header
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SYSTEMS))
def test_each_iteration_against_the_header(name, precision):
    s = system(name)
    mask = moving_mask(s)
    assert 0 < mask.sum() < s.num_particles
    ctx = prepared(name, precision)
    assert ctx.step_path()[0] == ("gather" if name == "drudes-at-the-end" else "tiled")
    ctx.minimize_begin(0.0, **GPU_FIRE)
    first = ctx.minimize_state()
    assert (first.iterations, first.uphill, first.since_uphill, first.converged, first.moving) == (0, 0, 0, 0, int(mask.sum()))
    assert (first.dt, first.alpha) == (PAR["dt_start"], PAR["alpha_start"]) and not work(ctx).any()
    st, branches = follow(ctx, mask, 3 if name == "water52430" else GPU_ITERATIONS, what=f"{name} {precision}")
    assert st.iterations == len(branches) and branches[0] == "first"
    if name == "water13":
        assert branches == [t.branch for t in gpu_trace(precision)]
        assert set(branches) == {"first", "mix", "grow", "uphill"}
    ctx.minimize_end()
    assert status_of(ctx.minimize_iterate) == _lib.ERR_STATE and status_of(ctx.minimize_state) == _lib.ERR_STATE
    ctx.close()


# ---- 2. one answer whatever the handle
def torch_harness(s, ctx):
    """the harness force law as a caller's call-out: elementwise fp64 torch, the same words whatever the handle"""
    torch = ctx.torch
    tethered = s.mass > 0
    tethered[s.pair_drude] = False
    t = torch.from_numpy(np.flatnonzero(tethered)).to(ctx.dev)
    pd, pp = (torch.from_numpy(np.ascontiguousarray(x, np.int64)).to(ctx.dev) for x in (s.pair_drude, s.pair_parent))
    x0 = ctx.x0[:, :3].to(torch.float64).clone()

    def force(c):
        x = c.posq[:, :3].to(torch.float64)
        if c.posq_corr is not None:
            x = x + c.posq_corr[:, :3].to(torch.float64)
        f = torch.zeros_like(x)
        f[t] = -synth.K_TETHER * (x[t] - x0[t])
        sep = x[pd] - x[pp]
        f[pd] = f[pd] - synth.K_DRUDE * sep
        f[pp] = f[pp] + synth.K_DRUDE * sep
        c.force.view(3, c.padded)[:, :c.n] = (f * TWO32).to(torch.int64).t()
    return force


@pytest.mark.parametrize("name", ["water52", "nacl"])
def test_one_answer_whatever_the_handle(name):
    s = system(name)
    want, paths = None, set()
    for mode, flags, stepped in (("TGNH", 0, False), ("TGNH", FLAG_WAVE_TILES, False), ("TGNH", FLAG_GATHER, False), ("dualNH", 0, False),
                                 ("TGNH", 0, True)):
        ctx = prepared(name, "mixed", flags=flags, mode=mode)
        paths.add(ctx.step_path()[0])
        if stepped:                                          # a handle that has taken steps and been flushed
            ctx.step(3)
            ctx.flush()
            dress(ctx, start(name))                          # (a step stores 0 in the w of posq_correction)
        ctx.force_fn = torch_harness(s, ctx)
        ctx.minimize_begin(0.0, **GPU_FIRE)
        ctx._minimize_batch(GPU_ITERATIONS)
        got = everything(ctx)
        ctx.minimize_end()
        want = got if want is None else want
        assert got == want, (mode, flags, stepped)
        ctx.close()
    assert paths == {"tiled", "gather"}


# ---- 3. masks
def test_masks():
    s = system("water52")
    n = s.num_particles
    rng = np.random.default_rng(5)
    callers = rng.random(n) < 0.4
    for kw in (dict(drude_only=True), dict(moving=callers), dict(moving=callers, drude_only=True)):
        mask = moving_mask(s, **kw)
        assert 0 < mask.sum() < (s.mass != 0).sum()
        ctx = prepared("water52")
        before = stored(ctx)
        ctx.minimize_begin(0.0, **kw, **GPU_FIRE)
        assert ctx.minimize_state().moving == mask.sum()
        follow(ctx, mask, 4, what=str(sorted(kw)))
        after = stored(ctx)
        for b, a in zip(before, after):                      # parents, massless slots, whatever the mask leaves out: bit for bit
            assert a[~mask].tobytes() == b[~mask].tobytes()
            assert (a[mask, :3] != b[mask, :3]).any(axis=1).all() and a[mask, 3].tobytes() == b[mask, 3].tobytes()
        assert not work(ctx)[:, ~mask].any()
        ctx.minimize_end()
        ctx.close()
    # a mask that leaves nothing
    ctx = prepared("water52")
    before = stored(ctx)
    nothing = np.zeros(n, bool)
    nothing[s.mass == 0] = True
    for kw in (dict(moving=nothing), dict(moving=np.zeros(n)), dict(moving=~moving_mask(s, drude_only=True), drude_only=True)):
        assert status_of(lambda: ctx.minimize_begin(**kw)) == _lib.ERR_STATE and "no slot moves" in ctx.lib.tgnh_last_error().decode()
        assert status_of(ctx.minimize_iterate) == _lib.ERR_STATE
    assert same(stored(ctx), before)
    ctx.close()


# ---- 4. what is left alone
def test_what_is_left_alone():
    ctx = prepared("water52")
    ctx.compute_forces()
    ctx.step(3)
    ctx.flush()
    p0 = stored(ctx)
    ctx.scale_positions(1.01, save=True)
    def rest():
        """everything of the handle that is no position (the queries first: they settle what a step left staged; bit 8, the sweep
        direction, is the harness force's to alternate)"""
        out = [ctx.velm.cpu().numpy().tobytes(), ctx.last_kinetic_energies().tobytes(), [ctx.thermostat_state(k).tobytes() for k in range(4)], ctx.time()]
        return out + [ctx.pending_state() & ~0x100]

    rest()
    kept = rest()
    moved = stored(ctx)
    ctx.minimize_begin(0.0, **GPU_FIRE)
    owed = ctx.pending_state()
    ctx.minimize_iterate()
    assert ctx.pending_state() == owed                       # (the harness force alternates bit 8, the sweep direction, itself: the minimiser's calls do not)
    ctx._minimize_batch(6)
    ctx.minimize_end()
    assert not same(stored(ctx), moved)
    assert rest() == kept
    ctx.restore_positions()
    assert same(stored(ctx), p0)                             # the snapshot of the earlier scale_positions(save=True)
    ctx.close()


def test_a_step_after_a_converged_minimisation():
    """... equals the step of a twin handle given the final positions by setPositions (fp64 positions: setPositions is exact)"""
    a, b = prepared("water52", "double"), prepared("water52", "double")
    st = a.minimizeEnergy()
    assert st.converged == 1 and 0 < st.iterations <= 2 * CONVERGES_AFTER
    final = stored(a)
    b.setPositions(coords(final))
    b.compute_forces()
    if (a.pending_state() ^ b.pending_state()) & 0x100:      # the harness force alternates the sweep direction: one more call-out evens it
        b.compute_forces()
    assert same(stored(b), final) and words(a).tobytes() == words(b).tobytes()      # a's buffer holds the forces of its final positions
    assert a.pending_state() == b.pending_state()
    for ctx in (a, b):
        ctx.step(1)
    assert state_bytes(a) == state_bytes(b) and not same(stored(a), final)
    a.close()
    b.close()


# ---- 5. convergence
def test_convergence_on_nacl():
    s = system("nacl")
    mask = moving_mask(s)
    ctx = prepared("nacl")
    st = ctx.minimizeEnergy()
    f = ctx.getForces()[mask]
    rms = float(np.sqrt((f * f).sum() / (3 * mask.sum())))
    print(f"nacl: converged {st.converged} after {st.iterations} iterations (the restatement: {CONVERGES_AFTER}), uphill {st.uphill}, "
          f"rms force {st.rms_force:.6g}, recomputed {rms:.6g}")
    assert st.converged == 1 and st.iterations <= 2 * CONVERGES_AFTER and st.moving == mask.sum()
    assert rms <= 10.0 and st.rms_force <= 10.0
    assert status_of(ctx.minimize_state) == _lib.ERR_STATE   # minimizeEnergy has ended it
    # a converged minimisation stays where it is
    ctx.setPositions(start("nacl"))
    ctx.minimize_begin()
    for _ in range(4):
        ctx._minimize_batch(50)
        if ctx.minimize_state().converged:
            break
    assert ctx.minimize_state().converged == 1
    held = everything(ctx)
    ctx._minimize_batch(20)
    assert everything(ctx) == held
    # a run that blew up stays as evidence
    ctx.setPositions(start("nacl"))
    ctx.minimize_begin()
    ctx._minimize_batch(3)
    slot = int(np.flatnonzero(mask)[7])
    ctx.minimize_work[1, slot] = float("nan")
    before, w0 = stored(ctx), work(ctx)
    ctx._minimize_batch(2)
    blown = ctx.minimize_state()
    assert blown.converged == -1 and blown.iterations == 3 and np.isnan(blown.power) and np.isnan(blown.vv) and np.isfinite(blown.ff)
    assert same(stored(ctx), before) and work(ctx).tobytes() == w0.tobytes()
    ctx.minimize_end()
    ctx.close()


# ---- 6. refusals on a live handle
def test_refusals_on_a_live_handle():
    torch = pytest.importorskip("torch")
    lib = _lib.load()
    # a DEFER_SCALE handle between steps
    ctx = prepared("water52", flags=FLAG_DEFER_SCALE)
    ctx.compute_forces()
    ctx.step(2)
    assert ctx.pending_state() & 0b101                       # a half kick is owed to velm
    held = stored(ctx)
    assert status_of(lambda: ctx.minimize_begin(0.0, **GPU_FIRE)) == _lib.ERR_STATE and "tgnh_flush" in lib.tgnh_last_error().decode()
    assert status_of(ctx.minimize_iterate) == _lib.ERR_STATE and same(stored(ctx), held)
    ctx.flush()
    assert ctx.pending_state() & 0b101 == 0
    ctx.minimize_begin(0.0, **GPU_FIRE)
    ctx._minimize_batch(2)
    ctx.step(1)                                              # ... and owes one again, with the minimisation under way
    assert ctx.pending_state() & 0b101
    held = everything(ctx)
    assert status_of(ctx.minimize_iterate) == _lib.ERR_STATE and "tgnh_flush" in lib.tgnh_last_error().decode()
    assert everything(ctx) == held
    ctx.minimize_end()
    ctx.close()
    # iterate before begin; mailboxes attached; begin on a capturing stream
    ctx = prepared("water52")
    held = stored(ctx)
    assert status_of(ctx.minimize_iterate) == _lib.ERR_STATE and "tgnh_minimize_begin" in lib.tgnh_last_error().decode()
    assert status_of(ctx.minimize_state) == _lib.ERR_STATE
    assert lib.tgnh_run_harness_minimize(ctx.h, ctx._x0_arg(), ctx.k_drude, ctx.k_tether, 2, ctx._stream()) == _lib.ERR_STATE
    _, ptr = ctx.exchange_create(1, 0)
    ctx.exchange_attach_pointers([ptr])
    assert status_of(lambda: ctx.minimize_begin(0.0, **GPU_FIRE)) == _lib.ERR_UNSUPPORTED and "mailbox" in lib.tgnh_last_error().decode()
    ctx.exchange_detach()
    ctx.minimize_begin(0.0, **GPU_FIRE)
    ctx.exchange_attach_pointers([ptr])
    assert status_of(ctx.minimize_iterate) == _lib.ERR_UNSUPPORTED
    ctx.exchange_detach()
    ctx.minimize_end()
    assert same(stored(ctx), held)
    d, _ = minimize_desc(ctx.n, 0.0, **GPU_FIRE)
    buf = torch.empty((3, ctx.n), dtype=torch.float64, device=ctx.dev)
    torch.cuda.synchronize(ctx.dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.tgnh_minimize_begin(ctx.h, C.byref(d), buf.data_ptr(), ctx._stream())
        message = lib.tgnh_last_error().decode()
        ctx.compute_forces()                                 # (something to record)
    torch.cuda.synchronize(ctx.dev)
    assert rc == _lib.ERR_STATE and "capturing" in message
    assert status_of(ctx.minimize_iterate) == _lib.ERR_STATE and same(stored(ctx), held)
    ctx.close()


# ---- 7. sharded, on one GPU
def test_two_shards_on_one_gpu():
    s = system("water52")
    mask = moving_mask(s)
    iterations = 8
    # the unsharded run, its sums and their restatement iteration by iteration
    full = prepared("water52")
    full.minimize_begin(0.0, **GPU_FIRE)
    sums, yard = [], []
    for _ in range(iterations):
        full.compute_forces()
        yard.append(fire_sums(words(full), work(full), mask))
        full.minimize_iterate()
        st = full.minimize_state()
        sums.append([st.power, st.ff, st.vv, float(st.moving)])
    want = stored(full)
    full.minimize_end()
    full.close()
    cut = 5 * 26                                             # cut at a molecule: slot 130, not a multiple of 64
    halves = [(0, cut), (cut, s.num_particles)]
    ranks = [context(s.slice_molecules(lo, hi), "mixed") for lo, hi in halves]
    for ctx, (lo, hi) in zip(ranks, halves):
        dress(ctx, start("water52")[lo:hi], lo)
    seen, calls, turn = [], [], [0]
    for k, ctx in enumerate(ranks):
        def allreduce(t, k=k, ctx=ctx):
            assert t.numel() == 4
            calls.append(k)
            seen.append(t.cpu().numpy().copy())
            t.copy_(ctx.torch.tensor(sums[turn[0]], dtype=ctx.torch.float64, device=ctx.dev))     # what a real all-reduce leaves on every rank
        ctx.set_allreduce(allreduce)
        ctx.minimize_begin(0.0, **GPU_FIRE)
    for it in range(iterations):
        turn[0] = it
        for ctx in ranks:
            ctx.compute_forces()
            ctx.minimize_iterate()
        for ctx in ranks:
            ctx.torch.cuda.synchronize(ctx.dev)
    assert calls == [0, 1] * iterations                       # 4 doubles, once per iteration and rank
    for it in range(iterations):
        a, b, y = seen[2 * it], seen[2 * it + 1], yard[it]
        eps = y.n * 2.0 ** -52
        total = a + b
        print(f"iteration {it}: shards' sums {total} against {sums[it]}")
        assert total[3] == y.n == mask.sum() and a[3] == mask[:cut].sum()
        for j, bound in enumerate((y.abs_P, y.abs_FF, y.abs_VV)):
            assert abs(total[j] - sums[it][j]) <= eps * bound, (it, j)
    out = [stored(ctx) for ctx in ranks]
    assert np.concatenate([o[0] for o in out]).tobytes() == want[0].tobytes()
    assert np.concatenate([o[1] for o in out]).tobytes() == want[1].tobytes()
    for ctx in ranks:
        assert ctx.minimize_state().iterations == iterations
        ctx.minimize_end()
        ctx.close()


# ---- 8. in a hipGraph
def test_iterations_replayed_from_a_graph():
    torch = pytest.importorskip("torch")
    eager = prepared("water52")
    eager.minimize_begin(0.0, **GPU_FIRE)
    eager._minimize_batch(10)
    want = everything(eager)
    eager.minimize_end()
    eager.close()
    ctx = prepared("water52")
    ctx.minimize_begin(0.0, **GPU_FIRE)                      # eagerly: the mask and the state block are uploaded outside the capture
    begun = everything(ctx)
    torch.cuda.synchronize(ctx.dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx._minimize_batch(10)
    torch.cuda.synchronize(ctx.dev)
    assert everything(ctx) == begun                          # a recording runs nothing
    g.replay()
    torch.cuda.synchronize(ctx.dev)
    got = everything(ctx)
    assert got == want and got[3] != begun[3]
    ctx.minimize_end()
    ctx.close()
