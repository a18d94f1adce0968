"""CPU tests of the minimiser (tgnh_minimize_begin, tgnh_minimize_iterate, tgnh_get_minimize_state, tgnh_minimize_end,
tgnh_run_harness_minimize): the yardstick, the inputs of the GPU tests, and the argument checks.

`fire_sums`, `fire_decide`, `fire_update` and `minimize` restate include/drude_tgnh.h's FIRE iteration in numpy -- per slot in
fp64, every product, quotient and sum rounded on its own, the per-slot terms added one after the other in slot order
(test_cm_motion.ordered_sum: a plain ordered sum), positions read and stored as tgnh_scale_positions reads and stores them -- and
are what tests/test_minimize_gpu.py holds the kernels against.  Beside each sum stands the sum of the absolute values of its
terms: two orders of adding n terms differ by less than n 2^-52 of it.

The harness force here (`harness_force_words`) is the library's force law in fp64 numpy; the device's kernel may contract a
product into the sum that follows, so its words can differ from these in the last place.  Nothing below or in the GPU tests needs
them equal: the GPU tests restate every iteration from the device's own force words, and only the BRANCHES a run takes are
compared between the two -- which is why the coverage test asserts that every decision's |P| stands a thousand times clear of its
summation bound."""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import (DrudeTGNHIntegrator, HostTopology, HipContext, MinimizeState, TgnhError, FIRE_DEFAULTS,
                                                   minimize_desc)
from test_cm_motion import ordered_sum

REAL = {"single": np.float32, "mixed": np.float32, "double": np.float64}
TWO32 = 4294967296.0

# what the GPU tests run with: a dt_max beyond the Drude spring's stability limit 2 / sqrt(k) = 3.1e-3, so that a run of 14
# iterations takes every branch
GPU_FIRE = dict(dt_start=2.5e-3, dt_max=5e-3, n_min=2, max_step=0.005)
GPU_ITERATIONS = 14
SEED = 20261019


def integ(chains=3):
    return DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, chains, True, True)


# ---- positions as the library keeps them ----
def split(pos, precision, w=None, cw=None):
    """fp64 coordinates [N, 3] -> (posq [N, 4], posq_correction [N, 4] or None) as Context::setPositions leaves them"""
    pos = np.asarray(pos, np.float64)
    posq = np.zeros((len(pos), 4), REAL[precision])
    posq[:, :3] = pos.astype(REAL[precision])
    if w is not None:
        posq[:, 3] = w
    corr = None
    if precision == "mixed":
        corr = np.zeros((len(pos), 4), np.float32)
        corr[:, :3] = (pos - posq[:, :3].astype(np.float64)).astype(np.float32)
        if cw is not None:
            corr[:, 3] = cw
    return posq, corr


def coords(stored):
    """x(i) as tgnh_scale_positions defines it: posq, plus posq_correction in mixed precision, each converted on its own"""
    posq, corr = stored
    x = posq[:, :3].astype(np.float64)
    return x if corr is None else x + corr[:, :3].astype(np.float64)


def moving_mask(system, drude_only=False, moving=None):
    mask = system.mass != 0
    if moving is not None:
        mask &= np.asarray(moving) != 0
    if drude_only:
        d = np.zeros(system.num_particles, bool)
        d[system.pair_drude] = True
        mask &= d
    return mask


def harness_force_words(x, x0, system, k_drude=synth.K_DRUDE, k_tether=synth.K_TETHER):
    """the harness force law -- a tether of every massive slot that is no Drude particle to its site, the Drude spring -- as
    fixed-point words [3, N]: (long long)(f * 2^32), truncated as the cast does"""
    f = np.zeros_like(x)
    tethered = system.mass > 0
    tethered[system.pair_drude] = False
    f[tethered] = -k_tether * (x[tethered] - x0[tethered])
    sep = x[system.pair_drude] - x[system.pair_parent]
    f[system.pair_drude] += -1.0 * k_drude * sep
    f[system.pair_parent] += k_drude * sep
    return np.ascontiguousarray(np.trunc(f * TWO32).astype(np.int64).T)


# ---- the header, restated ----
def new_state(par):
    return SimpleNamespace(iterations=0, uphill=0, since_uphill=0, converged=0, dt=float(par["dt_start"]), alpha=float(par["alpha_start"]),
                           power=0.0, ff=0.0, vv=0.0, rms_force=0.0, a=0.0, b=0.0)


def fire_sums(force, work, mask):
    """step 1: force int64 [3, N] words, work float64 [3, N], mask bool [N] -> P, FF, VV, moving and the sums of |term|"""
    f = force[:, mask].astype(np.float64) / TWO32
    v = np.asarray(work, np.float64)[:, mask]
    terms = np.stack([(f[0] * v[0] + f[1] * v[1]) + f[2] * v[2],
                      (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2],
                      (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]], 1)
    s, a = ordered_sum(terms), ordered_sum(np.abs(terms))
    return SimpleNamespace(P=float(s[0]), FF=float(s[1]), VV=float(s[2]), moving=float(mask.sum()), abs_P=float(a[0]), abs_FF=float(a[1]),
                           abs_VV=float(a[2]), n=int(mask.sum()))


def fire_decide(state, P, FF, VV, moving, par, tolerance):
    """step 3 -> (the new state, the branch taken: 'frozen', 'nan', 'converged', 'first', 'mix', 'grow' or 'uphill')"""
    st = SimpleNamespace(**vars(state))
    if st.converged != 0:
        return st, "frozen"
    with np.errstate(all="ignore"):
        rms = float(np.sqrt(np.float64(FF) / np.float64(3.0 * moving)))
    st.power, st.ff, st.vv, st.rms_force = P, FF, VV, rms
    if not all(math.isfinite(x) for x in (P, FF, VV, moving)):
        st.converged = -1
        return st, "nan"
    if rms <= tolerance:
        st.converged = 1
        return st, "converged"
    if st.iterations == 0:
        st.a, st.b, branch = 1.0, 0.0, "first"
    elif P > 0.0:
        st.since_uphill += 1
        st.a = 1.0 - st.alpha
        st.b = (st.alpha * math.sqrt(VV)) / math.sqrt(FF)
        branch = "mix"
        if st.since_uphill > par["n_min"]:
            st.dt = min(st.dt * par["f_inc"], par["dt_max"])
            st.alpha = st.alpha * par["f_alpha"]
            branch = "grow"
    else:
        st.uphill += 1
        st.since_uphill = 0
        st.a = st.b = 0.0
        st.dt = st.dt * par["f_dec"]
        st.alpha = par["alpha_start"]
        branch = "uphill"
    st.iterations += 1
    return st, branch


def fire_update(stored, work, force, mask, state, par):
    """step 4 -> ((posq, posq_correction), work, the mask of the slots whose displacement was capped); inputs untouched"""
    posq, corr = stored[0].copy(), None if stored[1] is None else stored[1].copy()
    work = np.array(work, np.float64)
    capped = np.zeros(len(mask), bool)
    if state.converged != 0:
        return (posq, corr), work, capped
    f = force[:, mask].astype(np.float64) / TWO32
    v = (state.a * work[:, mask]) + (state.b * f)
    v = v + state.dt * f
    d = state.dt * v
    r = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    over = r > par["max_step"]
    s = par["max_step"] / r[over]
    d[:, over] = d[:, over] * s
    capped[np.flatnonzero(mask)[over]] = True
    x = coords((posq[mask], None if corr is None else corr[mask])) + d.T
    hi = x.astype(posq.dtype)
    posq[mask, :3] = hi
    if corr is not None:
        corr[mask, :3] = (x - hi.astype(np.float64)).astype(np.float32)
    work[:, mask] = v
    return (posq, corr), work, capped


def minimize(system, stored, x0, mask, par, tolerance, iterations, stop=True):
    """`iterations` x {harness force, one iteration} -> (stored, work, state, trace); trace: one record per decision -- the
    sums, the branch, the capped slots.  stop: leave at the first decision that sets `converged`"""
    par = dict(FIRE_DEFAULTS, **par)
    work = np.zeros((3, system.num_particles))
    state, trace = new_state(par), []
    for _ in range(iterations):
        force = harness_force_words(coords(stored), x0, system)
        sums = fire_sums(force, work, mask)
        state, branch = fire_decide(state, sums.P, sums.FF, sums.VV, sums.moving, par, tolerance)
        stored, work, capped = fire_update(stored, work, force, mask, state, par)
        trace.append(SimpleNamespace(sums=sums, branch=branch, capped=capped, state=state))
        if stop and state.converged != 0:
            break
    return stored, work, state, trace


def displaced(system, seed=SEED):
    """the GPU tests' start: every slot that is no Drude particle displaced by N(0, 0.02 nm), every Drude particle displaced from
    its (displaced) parent by N(0, 0.003 nm)"""
    rng = np.random.default_rng(seed)
    pos = system.positions + rng.normal(0.0, 0.02, system.positions.shape)
    pos[system.pair_drude] = pos[system.pair_parent] + rng.normal(0.0, 0.003, (system.num_pairs, 3))
    return pos


def sites(system, precision):
    """the tether sites as HipContext.set_sites stores them: in the position type"""
    return system.positions.astype(REAL[precision]).astype(np.float64)


_cache = {}


def gpu_trace(precision):
    """the restatement's run of the GPU tests' 13-water case; computed once"""
    if precision not in _cache:
        s = synth.water_box(13)[0]
        _cache[precision] = minimize(s, split(displaced(s), precision), sites(s, precision), moving_mask(s), GPU_FIRE, 0.0, GPU_ITERATIONS)[3]
    return _cache[precision]


# ---- the yardstick's own checks ----
W = lambda *f: np.ascontiguousarray((np.array(f, np.float64) * TWO32).astype(np.int64).T)      # noqa: E731  forces [N, 3] -> words [3, N]


@pytest.mark.parametrize("precision", ["double", "mixed", "single"])
def test_by_hand(precision):
    """Two moving slots, three iterations -- first, P > 0 with growth and a capped step, P <= 0 -- in numbers whose every product,
    sum, quotient and root is exact in fp32: forces (3, 0, 0) and (0, 4, 0) twice, then reversed."""
    par = dict(dt_start=0.5, dt_max=1.0, max_step=4.5, f_inc=2.0, f_dec=0.5, alpha_start=0.5, f_alpha=0.5, n_min=0)
    mask = np.array([True, True])
    stored = split([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], precision, w=[0.25, -0.5])
    work, st = np.zeros((3, 2)), new_state(par)
    # iteration 0: v = 0; P = 0, FF = 9 + 16, VV = 0; a = 1, b = 0; v'' = dt f; d = dt v''
    f = W([3, 0, 0], [0, 4, 0])
    s = fire_sums(f, work, mask)
    assert (s.P, s.FF, s.VV, s.moving, s.abs_FF) == (0.0, 25.0, 0.0, 2.0, 25.0)
    st, branch = fire_decide(st, s.P, s.FF, s.VV, s.moving, par, 0.0)
    assert (branch, st.a, st.b, st.dt, st.alpha, st.iterations, st.rms_force) == ("first", 1.0, 0.0, 0.5, 0.5, 1, math.sqrt(25.0 / 6.0))
    stored, work, capped = fire_update(stored, work, f, mask, st, par)
    assert work.T.tolist() == [[1.5, 0, 0], [0, 2.0, 0]] and coords(stored).tolist() == [[0.75, 0, 0], [1, 2.0, 1]] and not capped.any()
    # iteration 1: P = 4.5 + 8, VV = 2.25 + 4; a = 0.5, b = (0.5 x 2.5) / 5; since_uphill = 1 > n_min: dt = 1, alpha = 0.25
    # v' = 0.5 v + 0.25 f = (1.5, 0, 0), (0, 2, 0); v'' = v' + 1 f = (4.5, 0, 0), (0, 6, 0); slot 1: r = 6 > 4.5, s = 0.75
    s = fire_sums(f, work, mask)
    assert (s.P, s.FF, s.VV, s.abs_P) == (12.5, 25.0, 6.25, 12.5)
    st, branch = fire_decide(st, s.P, s.FF, s.VV, s.moving, par, 0.0)
    assert (branch, st.a, st.b, st.dt, st.alpha, st.since_uphill, st.iterations) == ("grow", 0.5, 0.25, 1.0, 0.25, 1, 2)
    stored, work, capped = fire_update(stored, work, f, mask, st, par)
    assert work.T.tolist() == [[4.5, 0, 0], [0, 6.0, 0]] and capped.tolist() == [False, True]
    assert coords(stored).tolist() == [[5.25, 0, 0], [1, 6.5, 1]]
    # iteration 2: the forces reversed: P = -13.5 - 24 <= 0: a = b = 0, dt = 0.5, alpha back to 0.5; v'' = 0.5 f
    f = W([-3, 0, 0], [0, -4, 0])
    s = fire_sums(f, work, mask)
    assert (s.P, s.abs_P, s.VV) == (-37.5, 37.5, 56.25)
    st, branch = fire_decide(st, s.P, s.FF, s.VV, s.moving, par, 0.0)
    assert (branch, st.a, st.b, st.dt, st.alpha, st.uphill, st.since_uphill, st.iterations) == ("uphill", 0.0, 0.0, 0.5, 0.5, 1, 0, 3)
    stored, work, capped = fire_update(stored, work, f, mask, st, par)
    assert work.T.tolist() == [[-1.5, 0, 0], [0, -2.0, 0]] and coords(stored).tolist() == [[4.5, 0, 0], [1, 5.5, 1]]
    assert stored[0][:, 3].tolist() == [0.25, -0.5] and stored[0].dtype == REAL[precision]
    # the same three iterations with slot 1 masked out: it is untouched, and the sums are slot 0's
    mask = np.array([True, False])
    start = split([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]], precision)
    st = fire_decide(new_state(par), 0.0, 9.0, 0.0, 1.0, par, 0.0)[0]
    out, w1, _ = fire_update(start, np.zeros((3, 2)), W([3, 0, 0], [0, 4, 0]), mask, st, par)
    assert out[0][1].tobytes() == start[0][1].tobytes() and not w1[:, 1].any() and coords(out)[0].tolist() == [0.75, 0, 0]
    assert fire_sums(W([3, 0, 0], [0, 4, 0]), w1, mask).FF == 9.0


def test_the_decisions_that_end_a_run():
    par = dict(FIRE_DEFAULTS)
    st = new_state(par)
    done, branch = fire_decide(st, 0.0, 6.0 * 100.0, 0.0, 2.0, par, 10.0)             # rms = sqrt(600 / 6) = 10 <= 10
    assert (branch, done.converged, done.iterations, done.rms_force) == ("converged", 1, 0, 10.0)
    again, branch = fire_decide(done, 5.0, 1e9, 3.0, 2.0, par, 10.0)
    assert branch == "frozen" and vars(again) == vars(done)
    for bad in (np.nan, np.inf):
        blown, branch = fire_decide(st, 1.0, bad, 1.0, 2.0, par, 10.0)
        assert (branch, blown.converged, blown.iterations, blown.dt) == ("nan", -1, 0, st.dt)
    # a converged state moves nothing
    stored = split([[0.1, 0.2, 0.3]], "mixed")
    out, work, _ = fire_update(stored, np.ones((3, 1)), W([7, 7, 7]), np.array([True]), done, par)
    assert out[0].tobytes() == stored[0].tobytes() and out[1].tobytes() == stored[1].tobytes() and (work == 1.0).all()


@pytest.mark.parametrize("precision", ["double", "mixed", "single"])
def test_the_gpu_case_takes_every_branch(precision):
    """13 waters, GPU_FIRE, 14 iterations: every branch of the decision, capped and uncapped slots in iteration 0, and at every
    decision |P| at least 1000 x the bound on what another order of additions can change -- the device takes the same branches."""
    trace = gpu_trace(precision)
    assert len(trace) == GPU_ITERATIONS
    branches = [t.branch for t in trace]
    print(precision, branches, [f"{t.sums.P:.3g}" for t in trace])
    assert branches[0] == "first" and set(branches) == {"first", "mix", "grow", "uphill"}
    moving = moving_mask(synth.water_box(13)[0])
    assert moving.sum() == 52 and trace[0].capped[moving].any() and not trace[0].capped[moving].all()
    for k, t in enumerate(trace[1:], 1):
        bound = t.sums.n * 2.0 ** -52 * t.sums.abs_P
        assert abs(t.sums.P) >= 1000.0 * bound, (k, t.sums.P, bound)


def test_convergence_on_nacl():
    """Default parameters, synth.nacl() under the harness force from `displaced`, fp64 positions: the restatement converges
    (rms force <= 10 kJ/mol/nm) after 77 iterations (two of them uphill)."""
    s = synth.nacl()[0]
    mask = moving_mask(s)
    x0 = sites(s, "double")
    stored, work, st, trace = minimize(s, split(displaced(s), "double"), x0, mask, {}, 10.0, 2000)
    print("iterations", st.iterations, "rms", st.rms_force, "uphill", st.uphill)
    assert st.converged == 1 and st.iterations == len(trace) - 1 == CONVERGES_AFTER
    # the rms force recomputed from the final positions
    f = harness_force_words(coords(stored), x0, s)[:, mask].astype(np.float64) / TWO32
    assert np.sqrt((f * f).sum() / (3 * mask.sum())) <= 10.0
    # In the long run every sum falls.  FF: the largest value of each quarter of the run is below the quarter's before.  P and VV
    # start again from zero velocities after every reset and rise within each downhill stretch (the last one, along the soft tether
    # mode, is the longest), so for them the run is compared by halves: the largest |value| of the second half is below that of the first.
    series = {name: np.abs([getattr(t.sums, name) for t in trace]) for name in ("FF", "VV", "P")}
    quarters = [c.max() for c in np.array_split(series["FF"], 4)]
    assert all(quarters[j + 1] < quarters[j] for j in range(3)), quarters
    for name, v in series.items():
        first, second = np.array_split(v, 2)
        print(name, "first half max", first.max(), "second half max", second.max())
        assert second.max() < first.max(), name
    assert trace[-1].sums.FF < 1e-3 * trace[0].sums.FF


CONVERGES_AFTER = 77      # what test_convergence_on_nacl records; tests/test_minimize_gpu.py allows the device twice this


# ---- the binding and the entry points' argument checks (host-only handles, no GPU) ----
def test_the_binding_has_the_headers_layout():
    D, S = _lib.TgnhMinimizeDesc, _lib.TgnhMinimizeState
    assert C.sizeof(D) == 8 * 8 + 4 + 4 + 8 and (D.tolerance.offset, D.f_alpha.offset, D.n_min.offset, D.flags.offset, D.moving.offset) == (0, 56, 64, 68, 72)
    assert C.sizeof(S) == 4 * 8 + 4 + 4 + 6 * 8
    assert (S.iterations.offset, S.moving.offset, S.converged.offset, S.reserved.offset, S.dt.offset, S.rms_force.offset) == (0, 24, 32, 36, 40, 80)
    assert _lib.MIN_DRUDE_ONLY == 1
    d, mask = minimize_desc(3)
    assert mask is None and not d.moving and d.flags == 0
    assert (d.tolerance, d.dt_start, d.dt_max, d.max_step, d.f_inc, d.f_dec, d.alpha_start, d.f_alpha, d.n_min) == (10.0, 1e-4, 1e-3, 0.01, 1.1, 0.5, 0.1, 0.99, 5)
    d, mask = minimize_desc(3, 2.0, True, [0, 5, 0], n_min=7)
    assert mask.tolist() == [0, 1, 0] and d.moving == mask.ctypes.data and d.flags == 1 and d.n_min == 7 and d.tolerance == 2.0
    for bad in (dict(moving=[1, 1]), dict(stepsize=1.0)):
        with pytest.raises(TgnhError) as e:
            minimize_desc(3, **bad)
        assert e.value.status == _lib.ERR_ARG


BAD = [dict(tolerance=-1.0), dict(tolerance=np.nan), dict(dt_start=0.0), dict(dt_start=-1e-4), dict(dt_start=np.inf), dict(dt_max=5e-5),
       dict(dt_max=np.inf), dict(max_step=0.0), dict(max_step=np.nan), dict(f_inc=0.99), dict(f_inc=np.inf), dict(f_dec=0.0), dict(f_dec=1.0),
       dict(f_dec=np.nan), dict(f_alpha=0.0), dict(f_alpha=1.0), dict(alpha_start=0.0), dict(alpha_start=1.5), dict(alpha_start=np.nan),
       dict(n_min=-1)]


def test_argument_checks_through_a_host_only_handle():
    lib = _lib.load()
    s = synth.nacl()[0]
    top = HostTopology(s, integ(), mode="TGNH")
    work = C.c_void_p(4096)                                       # (never dereferenced: nothing launches)
    good, _ = minimize_desc(s.num_particles)
    st = _lib.TgnhMinimizeState()
    # a null handle
    assert lib.tgnh_minimize_begin(None, C.byref(good), work, None) == _lib.ERR_ARG
    assert lib.tgnh_minimize_iterate(None, None) == _lib.ERR_ARG
    assert lib.tgnh_get_minimize_state(None, None, C.byref(st)) == _lib.ERR_ARG
    assert lib.tgnh_minimize_end(None) == _lib.ERR_ARG
    assert lib.tgnh_run_harness_minimize(None, None, 1.0, 1.0, 1, None) == _lib.ERR_ARG
    # arguments, checked before the handle's own refusal
    assert lib.tgnh_minimize_begin(top.h, None, work, None) == _lib.ERR_ARG
    assert lib.tgnh_minimize_begin(top.h, C.byref(good), None, None) == _lib.ERR_ARG
    for bad in BAD:
        kw = dict(bad)
        d, _ = minimize_desc(s.num_particles, kw.pop("tolerance", 10.0), **kw)
        assert lib.tgnh_minimize_begin(top.h, C.byref(d), work, None) == _lib.ERR_ARG, bad
        assert b"tgnh_minimize_begin" in lib.tgnh_last_error()
    for flags in (2, 3, -1, 1 << 30):
        d, _ = minimize_desc(s.num_particles)
        d.flags = flags
        assert lib.tgnh_minimize_begin(top.h, C.byref(d), work, None) == _lib.ERR_ARG, flags
    assert lib.tgnh_get_minimize_state(top.h, None, None) == _lib.ERR_ARG
    assert lib.tgnh_run_harness_minimize(top.h, None, 1.0, 1.0, -1, None) == _lib.ERR_ARG
    # legal arguments: the refusal is the handle's (device -1: nothing launches)
    for d in (good, minimize_desc(s.num_particles, drude_only=True)[0], minimize_desc(s.num_particles, 0.0, dt_max=1e-4, alpha_start=1.0, f_inc=1.0, n_min=0)[0]):
        assert lib.tgnh_minimize_begin(top.h, C.byref(d), work, None) == _lib.ERR_STATE
    assert lib.tgnh_minimize_iterate(top.h, None) == _lib.ERR_STATE
    before = bytes(st)
    assert lib.tgnh_get_minimize_state(top.h, None, C.byref(st)) == _lib.ERR_STATE and bytes(st) == before
    assert lib.tgnh_run_harness_minimize(top.h, None, 1.0, 1.0, 3, None) == _lib.ERR_STATE
    assert lib.tgnh_minimize_end(top.h) == _lib.TGNH_OK and lib.tgnh_minimize_end(top.h) == _lib.TGNH_OK      # harmless without a begin
    top.close()


def test_the_result_object_is_read_only():
    st = _lib.TgnhMinimizeState()
    st.iterations, st.uphill, st.since_uphill, st.moving, st.converged = 77, 3, 4, 52, 1
    st.dt, st.alpha, st.power, st.ff, st.vv, st.rms_force = 1e-3, 0.05, 2.5, 100.0, 0.25, 9.5
    r = MinimizeState(st)
    assert (r.iterations, r.uphill, r.since_uphill, r.moving, r.converged) == (77, 3, 4, 52, 1)
    assert (r.dt, r.alpha, r.power, r.ff, r.vv, r.rms_force) == (1e-3, 0.05, 2.5, 100.0, 0.25, 9.5) and r.raw == bytes(st)
    assert "iterations=77" in repr(r)
    with pytest.raises(AttributeError):
        r.converged = 0
    with pytest.raises(AttributeError):
        r.extra = 1


def test_a_constrained_context_is_refused_without_a_mask():
    """minimizeEnergy's own check comes before anything touches the device: a context object without one shows it"""
    ctx = HipContext.__new__(HipContext)
    ctx.constrained = True
    with pytest.raises(TgnhError) as e:
        ctx.minimizeEnergy()
    assert e.value.status == _lib.ERR_STATE and "constraints" in str(e.value) and "drude_only" in str(e.value)
    ctx.h = None                                                  # (nothing for __del__ to close)
