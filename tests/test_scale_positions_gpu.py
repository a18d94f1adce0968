"""GPU tests of tgnh_scale_positions / tgnh_restore_positions (tgnh_scale_positions.hip) and of barostat.MonteCarloBarostat on a
HipContext, against `scaled` of tests/test_scale_positions.py: the header's formulas restated in numpy.

Positions: the systems' own, shifted by (3.1, -2.7, 0.4) nm -- centroids far from zero --, split into the stored types on the host,
with charges in posq.w and a pattern of its own in posq_correction.w, and written into the bound arrays as they are.  The scale is
anisotropic, (1.013, 0.991, 1.0007).

Tolerances, all formulas.
 * Molecules of n <= 64 members: the kernels add in the yardstick's order, so posq, posq_correction and both w are compared BIT FOR
   BIT.
 * n > 64: the kernel adds its members in another (fixed) order.  Two orders of n terms differ by less than n 2^-52 sum|x|; the
   centroid c = S / n by that over n (the division's own rounding, 2^-53 |c|, is inside the factor 2 between (n - 1) 2^-53 and
   n 2^-52); d = c (scale - 1) by |scale - 1| times that.  x' = x + d then differs by that bound plus one unit in the last place of
   the stored value at the yardstick's result -- the one rounding of the store, taken at a value that may sit on the other side of a
   rounding boundary: np.spacing in double and single precision; in mixed precision the stored value is hi + lo, whose last place is
   2^-24 of |lo| <= 2^-24 |x'|, so 2^-47 |x'| covers it.
 * Geometry: every member of a molecule receives the same d, so a difference of two members (a Drude particle and its parent, a slot
   and its molecule's first member) changes only by the roundings of the two results: each x' carries the fp64 addition's 2^-53 |x'|
   and the store's u |x'| (u = 2^-24 single, 2^-48 mixed -- lo is rounded to 24 bits of |x' - hi| <= 2^-24 |x'| --, 0 double).  Two of
   them at max|x'|: 2 (u + 2^-53) max|x'|.  At the largest single-precision box here (the polymer: max|x'| = 48.6 nm) that is
   5.8e-6 nm -- 3.7e-6 nm at 31 nm -- against a hard wall of 0.02 nm: the barostat's move does not reach the wall.
 * The barostat end to end: every molecule there has 5 members, so the positions of the device and of the stand-in are the same
   bits after every move; asked for is the value bound above, one unit in the last place per accepted move."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import (DrudeTGNHIntegrator, HipContext, TgnhError, create_handle, FLAG_DEFER_SCALE,
                                                   FLAG_WAVE_TILES, FLAG_TRUST_STATE_CHANGED, FLAG_GATHER)
from test_scale_positions import (scaled, arrays, coordinates, renumbered, centroids, StandIn, barostat_case, run_barostat, BOX, SHIFT,
                                  ANISO, REAL)

pytestmark = pytest.mark.gpu

PRECISIONS = ("double", "mixed", "single")
ULP_MIXED = 2.0 ** -47
U_STORE = {"single": 2.0 ** -24, "mixed": 2.0 ** -48, "double": 0.0}


def _water(n):
    return lambda: (synth.water_box(n)[0], None)


def _water26_64_65():
    s = synth.water_box(26)[0]
    labels = (np.arange(130) // 5).astype(np.int32)
    labels[:64] = -1                                        # 64 slots: the longest molecule the ordered sum serves
    labels[64:129] = -2                                     # 65: the shortest one a wavefront adds its own way
    return s, labels                                        # (slot 129, the last water's M site, keeps that water's label: a molecule of one)


def _water13_merged():
    s = synth.water_box(13)[0]
    labels = (np.arange(65) // 5).astype(np.int32)
    labels[60:] = 0                                         # waters 0 and 12: one molecule in two runs, n = 10
    return s, labels


def _drudes_at_the_end():
    from helpers import drudes_at_the_end
    return drudes_at_the_end(300)[0], None


# the smallest shapes at which each stage can go wrong
CASES = {"water1": (_water(1), PRECISIONS),                 # 5 slots: part of one wavefront
         "water13": (_water(13), PRECISIONS),               # 65: the 13th water must not be cut at lane 64
         "water52": (_water(52), PRECISIONS),               # 260: a second work-group
         "nacl": (lambda: (synth.nacl()[0], None), PRECISIONS),   # 2 500, molecules of 5 and 2 slots: spans of unequal molecules
         "water26-64-65": (_water26_64_65, PRECISIONS),     # the 64 / 65 boundary between the two sums; no pair is split
         "water13-merged": (_water13_merged, PRECISIONS),   # one molecule in two runs: the member lists, ascending order
         "drudes-at-the-end": (_drudes_at_the_end, PRECISIONS),   # members that are not consecutive, a gather-path handle
         "polymer": (lambda: (synth.polymer_in_water(300, 20)[0], None), PRECISIONS),   # one 900-slot molecule
         "water52430": (_water(52_430), ("mixed",))}        # 262 150 slots: past 1024 work-groups of either kind
_cache = {}


def case(name):
    """(system, labels [N] as the molecule table has them) -- built once"""
    if name not in _cache:
        s, labels = CASES[name][0]()
        _cache[name] = (s, np.ascontiguousarray(s.resid if labels is None else labels, np.int32), labels is not None)
    return _cache[name]


def start(name, precision):
    """(posq, corr) of the case before the move, in the stored types; built once and never changed"""
    key = (name, precision, "start")
    if key not in _cache:
        s = case(name)[0]
        rng = np.random.default_rng(5)
        posq, corr = arrays(s.positions + SHIFT, rng.uniform(-1.0, 1.0, s.num_particles), precision)
        for a in (posq, corr):
            if a is not None:
                a.setflags(write=False)
        _cache[key] = (posq, corr)
    return _cache[key]


def expected(name, precision):
    key = (name, precision, "scaled")
    if key not in _cache:
        _cache[key] = scaled(start(name, precision), case(name)[1], ANISO, precision)
    return _cache[key]


def integ(chains=3):
    return DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, chains, True, True)


def context(name, precision="mixed", flags=0, mode="TGNH"):
    s, labels, own = case(name)
    ctx = HipContext(s, integ(), mode=mode, precision=precision, flags=flags)
    if own:
        ctx.set_molecules(labels)
    return ctx


def load(ctx, pos_arrays):
    posq, corr = pos_arrays
    ctx.posq.copy_(ctx.torch.from_numpy(np.array(posq)).to(ctx.dev))            # (a copy: the cached arrays are read-only)
    if corr is not None:
        ctx.posq_corr.copy_(ctx.torch.from_numpy(np.array(corr)).to(ctx.dev))


def read(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    return ctx.posq.cpu().numpy(), None if ctx.posq_corr is None else ctx.posq_corr.cpu().numpy()


def state(pos_arrays):
    return pos_arrays[0].tobytes() + (b"" if pos_arrays[1] is None else pos_arrays[1].tobytes())


def status_of(fn):
    with pytest.raises(TgnhError) as e:
        fn()
    return e.value.status


# ---- 1. values, 2. geometry
@pytest.mark.parametrize("name,precision", [(n, p) for n, (_, ps) in CASES.items() for p in ps])
def test_against_the_header(name, precision):
    s, labels, _ = case(name)
    before, want = start(name, precision), expected(name, precision)
    mol = renumbered(labels)
    ctx = context(name, precision)
    assert ctx.num_molecules() == int(mol.max()) + 1 and np.array_equal(ctx.molecules(), mol)
    assert ctx.step_path()[0] == ("gather" if name == "drudes-at-the-end" else "tiled")
    load(ctx, before)
    ctx.scale_positions(ANISO)
    got = read(ctx)
    ctx.close()
    assert got[0].dtype == REAL[precision]
    assert got[0][:, 3].tobytes() == before[0][:, 3].tobytes()                      # the charges
    if precision == "mixed":
        assert got[1][:, 3].tobytes() == before[1][:, 3].tobytes()                  # posq_correction.w
    x0, xg, xw = coordinates(*before), coordinates(*got), coordinates(*want)
    assert np.abs(xw - x0).max() > 0.03                                             # (the shift: d is far from zero)
    S, c, n, A = centroids(x0, mol)
    short = (n <= 64)[mol]
    assert got[0][short].tobytes() == want[0][short].tobytes()                      # n <= 64: bit for bit
    if precision == "mixed":
        assert got[1][short].tobytes() == want[1][short].tobytes()
    if not short.all():                                                             # n > 64: the bound of the docstring
        long_ = ~short
        dd = (np.abs(np.array(ANISO) - 1.0) * (n[:, None] * 2.0 ** -52 * A / n[:, None]))[mol][long_]
        ulp = ULP_MIXED * np.abs(xw[long_]) if precision == "mixed" else np.spacing(np.abs(want[0][long_, :3])).astype(np.float64)
        err = np.abs(xg[long_] - xw[long_])
        print(f"{name} {precision}: molecules of n > 64: max |dx'| / (bound + ulp) = {(err / (dd + ulp)).max():.3e}")
        assert (err <= dd + ulp).all()
    assert (name in ("water26-64-65", "polymer")) == (not short.all())
    # geometry: Drude - parent, and every slot against its molecule's first member
    tol = 2.0 * (U_STORE[precision] + 2.0 ** -53) * np.abs(xg).max()
    first = np.r_[0, np.cumsum(n)[:-1]]
    first_slot = np.argsort(mol, kind="stable")[first][mol]
    pairs = np.abs((xg[s.pair_drude] - xg[s.pair_parent]) - (x0[s.pair_drude] - x0[s.pair_parent])).max() if s.num_pairs else 0.0
    intra = np.abs((xg - xg[first_slot]) - (x0 - x0[first_slot])).max()
    print(f"{name} {precision}: max|x'| {np.abs(xg).max():.3f} nm, geometry moved by {max(pairs, intra):.3e} nm, allowed {tol:.3e}")
    assert pairs <= tol and intra <= tol
    assert tol < 6e-6                                                               # (the docstring's figure: single precision, the polymer)


# ---- 3. the same bits across handles
@pytest.mark.parametrize("name", ["water52", "nacl", "water13-merged", "water26-64-65"])
def test_one_answer_whatever_the_handle(name):
    before = start(name, "mixed")
    want, paths = None, set()
    for mode, flags in (("TGNH", 0), ("TGNH", FLAG_GATHER), ("TGNH", FLAG_WAVE_TILES), ("dualNH", 0)):
        ctx = context(name, flags=flags, mode=mode)
        paths.add(ctx.step_path()[0])
        load(ctx, before)
        ctx.scale_positions(ANISO)
        got = state(read(ctx))
        load(ctx, before)
        ctx.scale_positions(ANISO)
        assert state(read(ctx)) == got, (mode, flags)                               # the same handle, the same positions, twice
        want = got if want is None else want
        assert got == want, (mode, flags)
        ctx.close()
    assert paths == {"tiled", "gather"}
    assert want == state(expected(name, "mixed")) or name == "water26-64-65"


# ---- 4. save / restore
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["nacl", "water13-merged"])
def test_save_and_restore(name, precision):
    before, want = start(name, precision), expected(name, precision)
    ctx = context(name, precision)
    load(ctx, before)
    assert status_of(ctx.restore_positions) == _lib.ERR_STATE                       # nothing saved yet
    ctx.scale_positions(ANISO, save=False)
    assert state(read(ctx)) == state(want)
    assert status_of(ctx.restore_positions) == _lib.ERR_STATE                       # still nothing
    load(ctx, before)
    ctx.scale_positions(ANISO, save=True)
    assert state(read(ctx)) == state(want)                                          # the same move with and without the snapshot
    ctx.restore_positions()
    assert state(read(ctx)) == state(before)                                        # bit for bit, both w included
    ctx.scale_positions(2.0)                                                        # (a scalar: isotropic) the snapshot outlives other moves
    assert state(read(ctx)) == state(scaled(before, case(name)[1], 2.0, precision))
    ctx.restore_positions()                                                         # a second restore
    assert state(read(ctx)) == state(before)
    # rebinding the positions invalidates it
    other = ctx.torch.zeros_like(ctx.posq)
    _lib_check = ctx.lib.tgnh_bind_buffers(ctx.h, other.data_ptr(), ctx.posq_corr.data_ptr() if ctx.posq_corr is not None else None,
                                           ctx.velm.data_ptr(), ctx.force.data_ptr(), ctx.pos_delta.data_ptr())
    assert _lib_check == _lib.TGNH_OK
    assert status_of(ctx.restore_positions) == _lib.ERR_STATE and "rebound" in ctx.lib.tgnh_last_error().decode()
    assert ctx.lib.tgnh_bind_buffers(ctx.h, ctx.posq.data_ptr(), ctx.posq_corr.data_ptr() if ctx.posq_corr is not None else None,
                                     ctx.velm.data_ptr(), ctx.force.data_ptr(), ctx.pos_delta.data_ptr()) == _lib.TGNH_OK
    assert status_of(ctx.restore_positions) == _lib.ERR_STATE                       # bound back: the snapshot stays invalid
    ctx.scale_positions(ANISO, save=True)
    ctx.restore_positions()
    assert state(read(ctx)) == state(before)
    ctx.close()


def test_a_trial_move_recorded_into_a_graph():
    before, want = start("nacl", "mixed"), expected("nacl", "mixed")
    ctx = context("nacl")
    torch = ctx.torch
    load(ctx, before)
    ctx.scale_positions(ANISO, save=True)                                           # outside the capture: device tables and the snapshot exist
    ctx.restore_positions()
    torch.cuda.synchronize(ctx.dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.scale_positions(ANISO, save=True)
    torch.cuda.synchronize(ctx.dev)
    assert state(read(ctx)) == state(before)                                        # a recording runs nothing
    g.replay()
    assert state(read(ctx)) == state(want)
    ctx.restore_positions()
    assert state(read(ctx)) == state(before)
    ctx.close()


# ---- 5. the trajectory is untouched
def whole_state(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    out = [ctx.posq.cpu().numpy().tobytes(), ctx.velm.cpu().numpy().tobytes(), ctx.force.cpu().numpy().tobytes()]
    if ctx.posq_corr is not None:
        out.append(ctx.posq_corr.cpu().numpy().tobytes())
    return out + [ctx.thermostat_state(k).tobytes() for k in range(4)] + [repr(ctx.time())]


def test_the_trajectory_is_untouched():
    a, b = context("water52", flags=FLAG_TRUST_STATE_CHANGED), context("water52", flags=FLAG_TRUST_STATE_CHANGED)
    for ctx in (a, b):
        ctx.step(3)
    assert whole_state(a) == whole_state(b)
    owed, velm = a.pending_state(), a.velm.cpu().numpy().tobytes()
    assert owed & (1 << 9)                                                          # the next half would start from the carried sums
    a.scale_positions(ANISO)
    assert a.pending_state() == owed == b.pending_state()
    assert a.compute_kinetic_energies().tobytes() == b.compute_kinetic_energies().tobytes()     # after the move, and without one
    owed = a.pending_state()
    assert owed == b.pending_state()
    assert a.velm.cpu().numpy().tobytes() == velm
    assert a.posq.cpu().numpy().tobytes() != b.posq.cpu().numpy().tobytes()
    # the twin receives the moved positions through its bound arrays; both recompute their forces, as the header asks
    b.posq.copy_(a.posq)
    b.posq_corr.copy_(a.posq_corr)
    assert b.pending_state() == owed
    for ctx in (a, b):
        ctx.compute_forces()
        ctx.step(5)
    assert whole_state(a) == whole_state(b)
    assert a.pending_state() == b.pending_state() and a.status_flags() == 0
    a.close(); b.close()


# ---- 6. a handle that owes a half kick
def test_a_deferred_handle_refuses_until_flushed():
    before = start("water52", "mixed")
    ctx = context("water52", flags=FLAG_DEFER_SCALE)
    load(ctx, before)
    ctx.scale_positions(ANISO)                                                      # before the first step: nothing is owed
    assert state(read(ctx)) == state(expected("water52", "mixed"))
    load(ctx, before)
    ctx.compute_forces()
    ctx.step(2)
    assert ctx.pending_state() & 0b101                                              # a half kick is owed to velm
    held = read(ctx)
    assert status_of(lambda: ctx.scale_positions(ANISO, save=True)) == _lib.ERR_STATE and "tgnh_flush" in ctx.lib.tgnh_last_error().decode()
    assert state(read(ctx)) == state(held)
    assert status_of(ctx.restore_positions) == _lib.ERR_STATE                       # ... and nothing was saved
    ctx.flush()
    assert ctx.pending_state() & 0b101 == 0
    ctx.scale_positions(ANISO, save=True)
    assert state(read(ctx)) == state(scaled(held, case("water52")[1], ANISO, "mixed"))
    ctx.restore_positions()
    assert state(read(ctx)) == state(held)
    ctx.close()


# ---- 7. arguments on a device handle
def test_arguments_on_a_device_handle():
    before = start("water13", "mixed")
    ctx = context("water13")
    load(ctx, before)
    lib = ctx.lib
    assert lib.tgnh_scale_positions(ctx.h, None, 0, ctx._stream()) == _lib.ERR_ARG
    for k in range(3):
        for v in (0.0, -1.0, np.nan, np.inf, -np.inf):
            odd = (C.c_double * 3)(1.0, 1.0, 1.0)
            odd[k] = v
            assert lib.tgnh_scale_positions(ctx.h, odd, 1, ctx._stream()) == _lib.ERR_ARG, (k, v)
    assert status_of(lambda: ctx.scale_positions((1.0, 1.0))) == _lib.ERR_ARG
    assert status_of(ctx.restore_positions) == _lib.ERR_STATE                       # no refused call has saved anything
    assert state(read(ctx)) == state(before)
    # labels that split a pair: refused, and the table in force keeps working
    s, labels, _ = case("water13")
    odd = labels.copy()
    odd[s.pair_drude[3]] = 77
    assert status_of(lambda: ctx.set_molecules(odd)) == _lib.ERR_ARG
    ctx.scale_positions(ANISO)
    assert state(read(ctx)) == state(expected("water13", "mixed"))
    # a new table on a live handle: the device tables follow
    merged = case("water13-merged")[1]
    ctx.set_molecules(merged)
    load(ctx, before)
    ctx.scale_positions(ANISO)
    assert state(read(ctx)) == state(expected("water13-merged", "mixed"))
    ctx.set_molecules(None)
    load(ctx, before)
    ctx.scale_positions(ANISO)
    assert state(read(ctx)) == state(expected("water13", "mixed"))
    ctx.close()


def test_unbound_buffers():
    s = case("water13")[0]
    lib = _lib.load()
    i = integ()
    group, ngroups = i._resolve_groups(s.num_particles)
    h = create_handle(lib, s, i, group, ngroups, _lib.MODE_TGNH, _lib.PREC_MIXED, 0, 0, synth.KB, (s.num_particles + 31) // 32 * 32)
    ok = (C.c_double * 3)(*ANISO)
    assert lib.tgnh_scale_positions(h, ok, 0, None) == _lib.ERR_STATE and b"tgnh_bind_buffers" in lib.tgnh_last_error()
    assert lib.tgnh_restore_positions(h, None) == _lib.ERR_STATE
    assert lib.tgnh_set_molecules(h, None) == _lib.TGNH_OK                          # the table needs no buffers
    assert lib.tgnh_destroy(h) == _lib.TGNH_OK


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_handle_without_pairs(precision):
    s = synth.DrudeSystem(mass=np.array([12.0, 1.0, 0.0]), pair_drude=np.zeros(0, np.int32), pair_parent=np.zeros(0, np.int32),
                          resid=np.zeros(3, np.int32), positions=np.arange(9.0).reshape(3, 3) / 7.0, velocities=np.zeros((3, 3)))
    ctx = HipContext(s, integ(), precision=precision)
    before = arrays(s.positions + SHIFT, [0.1, -0.2, 0.3], precision)
    load(ctx, before)
    assert ctx.num_molecules() == 1
    ctx.scale_positions(ANISO, save=True)
    assert state(read(ctx)) == state(scaled(before, s.resid, ANISO, precision))
    ctx.restore_positions()
    assert state(read(ctx)) == state(before)
    ctx.close()


# ---- 8. the barostat end to end
class Recorded:
    """a HipContext for the barostat, with what the stand-in offers the test: state() -- the arrays' bits"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __getattr__(self, name):
        return getattr(self.ctx, name)

    def state(self):
        return state(read(self.ctx))


def test_the_barostat_end_to_end():
    s, mol, x, energy = barostat_case(2.0)
    ctx = HipContext(s, integ(), precision="mixed")
    first = arrays(x, np.zeros(len(x)), "mixed")
    load(ctx, first)
    twin = StandIn(x, np.zeros(len(x)), s.resid, "mixed")
    assert twin.state() == state(first)
    want_acc, _, want_box, _ = run_barostat(twin, energy, 20, 11, BOX)
    acc, _, box, baro = run_barostat(Recorded(ctx), energy, 20, 11, BOX)            # (asserts: a rejected move leaves the arrays bit for bit)
    print(f"accepted {sum(acc)} of 20: {''.join('+' if a else '-' for a in acc)}")
    assert acc == want_acc and box.tolist() == want_box.tolist()
    assert True in acc and False in acc
    err = np.abs(ctx.getPositions() - twin.getPositions())
    assert (err <= sum(acc) * ULP_MIXED * np.abs(twin.getPositions())).all()
    # one more move, made to be rejected: an energy that soars with the second call
    calls = [0]

    def soaring(c):
        calls[0] += 1
        return energy(c) + (1e9 if calls[0] % 2 == 0 else 0.0)
    held = state(read(ctx))
    box2, ok = baro.update(ctx, box, soaring)
    assert not ok and box2.tolist() == box.tolist() and state(read(ctx)) == held
    ctx.close()
