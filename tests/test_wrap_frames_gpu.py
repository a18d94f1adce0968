"""GPU tests of tgnh_wrap_molecules and tgnh_write_frame (tgnh_wrap.hip) against `wrapped` and `frame_of` of tests/test_wrap_frames.py:
the header's formulas restated in numpy.

Inputs: the cases of tests/test_scale_positions_gpu.py -- the smallest shapes at which each stage can go wrong --, their positions
shifted by (-0.47, -0.53, -0.37) nm, in the triclinic box a = (0.83, 0, 0), b = (0.17, 0.71, 0), c = (-0.29, 0.23, 0.97) nm; in mixed
precision every second molecule carries a hi / lo split no store would choose (test_wrap_frames.inputs).

EVERY COMPARISON OF VALUES IS BIT FOR BIT.  Cell indices are integers and d is formed from them and the box alone, so once a centroid
falls in the yardstick's cell every stored value is the yardstick's, for molecules of more than 64 members too (whose sum the kernel
takes in another order: below 6e-9 of a cell edge, against a margin of at least 1e-4 that tests/test_wrap_frames.py asserts for
every case used here).
Geometry: every member of a molecule receives the same d, so a difference of two members changes only by the roundings of the two
results, 2 (u + 2^-53) max|x'| with u = 2^-24 single, 2^-48 mixed, 0 double: test_scale_positions_gpu's derived bound."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import (DrudeTGNHIntegrator, HipContext, TgnhError, FLAG_DEFER_SCALE, FLAG_WAVE_TILES,
                                                   FLAG_TRUST_STATE_CHANGED, FLAG_GATHER)
from test_scale_positions import centroids, renumbered, coordinates, arrays, REAL
from test_scale_positions_gpu import CASES, case, context, load, read, state
from test_wrap_frames import wrapped, frame_of, inputs, desc, integ, BOX, WSHIFT, WRAP, SKIP_DRUDE, INTERLEAVED

pytestmark = pytest.mark.gpu

U_STORE = {"single": 2.0 ** -24, "mixed": 2.0 ** -48, "double": 0.0}
SENTINEL = np.float32(-12345.5)
_cache = {}


def start(name, precision):
    """the case's arrays before anything is done to them; built once and never changed"""
    key = (name, precision, "start")
    if key not in _cache:
        posq, corr = inputs(name, precision)
        for a in (posq, corr):
            if a is not None:
                a.setflags(write=False)
        _cache[key] = (posq, corr)
    return _cache[key]


def expected(name, precision):
    key = (name, precision, "wrapped")
    if key not in _cache:
        _cache[key] = wrapped(start(name, precision), case(name)[1], BOX, precision)
    return _cache[key]


def expected_frame(name, precision, flags, unit):
    key = (name, precision, flags & (WRAP | SKIP_DRUDE), unit)
    if key not in _cache:
        s, labels, _ = case(name)
        _cache[key] = frame_of(start(name, precision), labels, s.pair_drude, BOX, flags, unit, precision)
    return _cache[key]


def boxed(name, precision="mixed", flags=0, mode="TGNH"):
    ctx = context(name, precision, flags=flags, mode=mode)
    ctx.setPeriodicBoxVectors(*BOX)
    load(ctx, start(name, precision))
    return ctx


def status_of(fn):
    with pytest.raises(TgnhError) as e:
        fn()
    return e.value.status


def raw_frame(ctx, flags, unit=1.0, pad=7, tail=64):
    """tgnh_write_frame into a buffer full of SENTINEL -> (status, the buffer on the host, count, stride); planar frames get a stride of
    count + pad, and `tail` floats lie beyond the capacity"""
    torch = ctx.torch
    count = ctx.frame_count(bool(flags & SKIP_DRUDE))
    d = desc(flags, count, unit, stride=None if flags & INTERLEAVED else count + pad)
    buf = torch.full((d.capacity + tail,), float(SENTINEL), dtype=torch.float32, device=ctx.dev)
    rc = ctx.lib.tgnh_write_frame(ctx.h, C.byref(d), buf.data_ptr(), ctx._stream())
    torch.cuda.synchronize(ctx.dev)
    return rc, buf.cpu().numpy(), count, d.stride


def laid_out(frame, flags, count, stride, size):
    """float32 [count, 3] as the buffer must hold it, SENTINEL everywhere else"""
    want = np.full(size, SENTINEL, np.float32)
    if flags & INTERLEAVED:
        want[:3 * count] = frame.reshape(-1)
    else:
        for k in range(3):
            want[k * stride:k * stride + count] = frame[:, k]
    return want


# ---- 1. wrap_molecules against the header
@pytest.mark.parametrize("name,precision", [(n, p) for n, (_, ps) in CASES.items() for p in ps])
def test_wrap_against_the_header(name, precision):
    s, labels, _ = case(name)
    before, want = start(name, precision), expected(name, precision)
    mol = renumbered(labels)
    ctx = boxed(name, precision)
    assert ctx.step_path()[0] == ("gather" if name == "drudes-at-the-end" else "tiled")
    assert ctx.getPeriodicBoxVectors().tobytes() == BOX.tobytes()
    ctx.wrap_molecules()
    got = read(ctx)
    ctx.close()
    assert got[0].dtype == REAL[precision]
    assert got[0].tobytes() == want[0].tobytes()                                    # posq, w included: bit for bit
    if precision == "mixed":
        assert got[1].tobytes() == want[1].tobytes()                                # posq_correction: the molecules that stay keep their split
    assert state(got) != state(before)
    x0, xg = coordinates(*before), coordinates(*got)
    S, c, n, A = centroids(x0, mol)
    tol = 2.0 * (U_STORE[precision] + 2.0 ** -53) * np.abs(xg).max()
    first = np.r_[0, np.cumsum(n)[:-1]]
    first_slot = np.argsort(mol, kind="stable")[first][mol]
    pairs = np.abs((xg[s.pair_drude] - xg[s.pair_parent]) - (x0[s.pair_drude] - x0[s.pair_parent])).max() if s.num_pairs else 0.0
    intra = np.abs((xg - xg[first_slot]) - (x0 - x0[first_slot])).max()
    print(f"{name} {precision}: max|x'| {np.abs(xg).max():.3f} nm, geometry moved by {max(pairs, intra):.3e} nm, allowed {tol:.3e}")
    assert pairs <= tol and intra <= tol
    cg = centroids(xg, mol)[1]                                                      # every centre lies in [0, ax) x [0, by) x [0, cz) now
    assert (cg > -1e-6).all() and (cg < np.diag(BOX) + 1e-6).all()


# ---- 2. the same bits across handles
@pytest.mark.parametrize("name", ["water52", "nacl", "water13-merged", "water26-64-65"])
def test_one_answer_whatever_the_handle(name):
    before, want = start(name, "mixed"), state(expected(name, "mixed"))
    wf = expected_frame(name, "mixed", WRAP | SKIP_DRUDE, 10.0)
    paths = set()
    for mode, flags in (("TGNH", 0), ("TGNH", FLAG_GATHER), ("TGNH", FLAG_WAVE_TILES), ("dualNH", 0)):
        ctx = boxed(name, flags=flags, mode=mode)
        paths.add(ctx.step_path()[0])
        for _ in range(2):                                                          # the same handle, the same positions, twice
            load(ctx, before)
            f = ctx.frame(wrap=True, skip_drude=True, unit=10.0).cpu().numpy()
            assert f.tobytes() == wf.tobytes(), (mode, flags)
            ctx.wrap_molecules()
            assert state(read(ctx)) == want, (mode, flags)
        ctx.close()
    assert paths == {"tiled", "gather"}


# ---- 3. write_frame against the header
FRAME_CASES = [(n, p) for n in ("water13", "nacl", "water13-merged", "polymer", "drudes-at-the-end") for p in CASES[n][1]] + [("water52430", "mixed")]


@pytest.mark.parametrize("name,precision", FRAME_CASES)
def test_frames_against_the_header(name, precision):
    before = start(name, precision)
    ctx = boxed(name, precision)
    velm = ctx.velm.cpu().numpy().tobytes()
    seen = set()
    for flags in range(8):
        for unit in (1.0, 10.0):
            rc, buf, count, stride = raw_frame(ctx, flags, unit)
            assert rc == _lib.TGNH_OK, (flags, unit, ctx.lib.tgnh_last_error())
            want = expected_frame(name, precision, flags, unit)
            assert want.shape == (count, 3)
            assert buf.tobytes() == laid_out(want, flags, count, stride, len(buf)).tobytes(), (flags, unit)    # gaps and tail keep the sentinel
            seen.add(buf.tobytes())
    assert len(seen) == 16                                                          # no two of them are the same frame
    assert state(read(ctx)) == state(before) and ctx.velm.cpu().numpy().tobytes() == velm
    # the Python surface lays out the same values
    f = ctx.frame(wrap=True, skip_drude=True, unit=10.0, planes=True)
    assert f.dtype == ctx.torch.float32 and f.device == ctx.posq.device
    assert f.cpu().numpy().tobytes() == np.ascontiguousarray(expected_frame(name, precision, WRAP | SKIP_DRUDE, 10.0).T).tobytes()
    out = ctx.torch.zeros((ctx.n, 3), dtype=ctx.torch.float32, device=ctx.dev)
    assert ctx.frame(out=out) is out and out.cpu().numpy().tobytes() == expected_frame(name, precision, 0, 1.0).tobytes()
    ctx.close()


# ---- 4. the frame of a wrap is the wrap's frame
@pytest.mark.parametrize("name", ["nacl", "water13-merged", "polymer", "drudes-at-the-end"])
def test_the_wrapped_frame_is_the_frame_after_the_wrap(name):
    ctx = boxed(name, "double")
    f = ctx.frame(wrap=True, unit=10.0).cpu().numpy()
    ctx.wrap_molecules()
    assert ctx.frame(wrap=False, unit=10.0).cpu().numpy().tobytes() == f.tobytes()
    assert ctx.frame(wrap=True, unit=10.0).cpu().numpy().tobytes() == f.tobytes()  # ... and a second wrap has nothing to move
    held = state(read(ctx))
    ctx.wrap_molecules()
    assert state(read(ctx)) == held
    ctx.close()


# ---- 5. a hipGraph
def test_recorded_into_a_graph():
    before, want = start("nacl", "mixed"), expected("nacl", "mixed")
    wf = expected_frame("nacl", "mixed", WRAP, 10.0)
    ctx = boxed("nacl")                                                             # (the default table: nothing of it is on the device yet)
    torch = ctx.torch
    a = torch.full((ctx.n, 3), float(SENTINEL), dtype=torch.float32, device=ctx.dev)
    b = torch.full((3, ctx.frame_count(True)), float(SENTINEL), dtype=torch.float32, device=ctx.dev)
    ticks = torch.zeros(1, device=ctx.dev)
    torch.cuda.synchronize(ctx.dev)
    g0 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g0):
        ticks.add_(1.0)
        first = [status_of(ctx.wrap_molecules), status_of(lambda: ctx.frame(wrap=True, unit=10.0, out=a)),
                 status_of(lambda: ctx.frame(skip_drude=True, planes=True, out=b))]
        messages = ctx.lib.tgnh_last_error().decode()
    g0.replay()
    torch.cuda.synchronize(ctx.dev)
    assert first == [_lib.ERR_STATE] * 3 and "capturing" in messages
    assert state(read(ctx)) == state(before)                                        # ... and nothing was written
    assert (a.cpu().numpy() == SENTINEL).all() and (b.cpu().numpy() == SENTINEL).all()
    # once outside the capture: the tables exist
    ctx.wrap_molecules()
    ctx.frame(skip_drude=True, planes=True, out=b)
    load(ctx, before)
    b.fill_(float(SENTINEL))
    torch.cuda.synchronize(ctx.dev)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ctx.frame(wrap=True, unit=10.0, out=a)
        ctx.wrap_molecules()
        ctx.frame(skip_drude=True, planes=True, out=b)
    torch.cuda.synchronize(ctx.dev)
    assert state(read(ctx)) == state(before) and (a.cpu().numpy() == SENTINEL).all()      # a recording runs nothing
    g.replay()
    assert state(read(ctx)) == state(want)
    assert a.cpu().numpy().tobytes() == wf.tobytes()
    plain = frame_of(want, case("nacl")[1], case("nacl")[0].pair_drude, None, SKIP_DRUDE, 1.0, "mixed")
    assert b.cpu().numpy().tobytes() == np.ascontiguousarray(plain.T).tobytes()
    load(ctx, before)                                                               # the graph again, from the same positions
    g.replay()
    assert state(read(ctx)) == state(want)
    ctx.close()


# ---- 6. the trajectory is untouched
def rest_of_state(ctx):
    ctx.torch.cuda.synchronize(ctx.dev)
    return [ctx.velm.cpu().numpy().tobytes(), ctx.force.cpu().numpy().tobytes()] + [ctx.thermostat_state(k).tobytes() for k in range(4)] + \
           [repr(ctx.time()), ctx.pending_state()]


def test_the_trajectory_is_untouched():
    a, b = context("water52", flags=FLAG_TRUST_STATE_CHANGED), context("water52", flags=FLAG_TRUST_STATE_CHANGED)
    for ctx in (a, b):
        ctx.step(3)
    assert rest_of_state(a) == rest_of_state(b) and state(read(a)) == state(read(b))
    owed = a.pending_state()
    assert owed & (1 << 9)                                                          # the next half would start from the carried sums
    a.setPeriodicBoxVectors(*BOX)
    held = read(a)
    f = a.frame(wrap=True, skip_drude=True, unit=10.0)
    assert state(read(a)) == state(held)                                            # a frame writes no position
    a.wrap_molecules()
    assert state(read(a)) == state(wrapped(held, case("water52")[1], BOX, "mixed")) != state(held)
    assert a.frame(skip_drude=True, unit=10.0).cpu().numpy().tobytes() == f.cpu().numpy().tobytes()
    assert rest_of_state(a) == rest_of_state(b)                                     # pending_state, velm, the thermostat: the same bits
    assert a.compute_kinetic_energies().tobytes() == b.compute_kinetic_energies().tobytes()
    assert a.pending_state() == b.pending_state() and a.status_flags() == 0
    a.close(); b.close()


def test_a_handle_that_owes_a_half_kick_accepts_both():
    ctx = context("water52", flags=FLAG_DEFER_SCALE)
    ctx.setPeriodicBoxVectors(*BOX)
    load(ctx, start("water52", "mixed"))
    ctx.compute_forces()
    ctx.step(2)
    assert ctx.pending_state() & 0b101                                              # a half kick is owed to velm
    held, rest = read(ctx), rest_of_state(ctx)                                      # (reading the thermostat settles the chain it still owed ...)
    owed = ctx.pending_state()
    assert owed & 0b101                                                             # (... and leaves the kick owed)
    labels, drudes = case("water52")[1], case("water52")[0].pair_drude
    f = ctx.frame(wrap=True, unit=10.0).cpu().numpy()
    assert f.tobytes() == frame_of(held, labels, drudes, BOX, WRAP, 10.0, "mixed").tobytes()
    ctx.wrap_molecules()
    assert state(read(ctx)) == state(wrapped(held, labels, BOX, "mixed"))
    assert ctx.pending_state() == owed and rest_of_state(ctx) == rest
    ctx.close()


# ---- 7. arguments on a device handle
def test_arguments_on_a_device_handle():
    before = start("water13", "mixed")
    ctx = context("water13")
    load(ctx, before)
    lib = ctx.lib
    s, labels, _ = case("water13")
    # no box: the wrap and a wrapped frame are refused, a plain frame works
    assert ctx.getPeriodicBoxVectors() is None
    assert status_of(ctx.wrap_molecules) == _lib.ERR_STATE and "box" in lib.tgnh_last_error().decode()
    assert status_of(lambda: ctx.frame(wrap=True)) == _lib.ERR_STATE and "box" in lib.tgnh_last_error().decode()
    assert ctx.frame().cpu().numpy().tobytes() == frame_of(before, labels, s.pair_drude, None, 0, 1.0, "mixed").tobytes()
    assert status_of(lambda: ctx.setPeriodicBoxVectors((1, 0, 0), (0.6, 1, 0), (0, 0, 1))) == _lib.ERR_ARG
    assert ctx.getPeriodicBoxVectors() is None
    ctx.setPeriodicBoxVectors(*BOX)
    # capacity one float short: refused with out untouched
    for flags in (0, WRAP | SKIP_DRUDE, INTERLEAVED, WRAP | INTERLEAVED):
        count = ctx.frame_count(bool(flags & SKIP_DRUDE))
        d = desc(flags, count)
        d.capacity -= 1
        buf = ctx.torch.full((3 * count + 8,), float(SENTINEL), dtype=ctx.torch.float32, device=ctx.dev)
        assert lib.tgnh_write_frame(ctx.h, C.byref(d), buf.data_ptr(), ctx._stream()) == _lib.ERR_ARG and b"capacity" in lib.tgnh_last_error()
        assert (buf.cpu().numpy() == SENTINEL).all()
    assert status_of(lambda: ctx.frame(out=ctx.torch.zeros((ctx.n, 3), dtype=ctx.torch.float64, device=ctx.dev))) == _lib.ERR_ARG
    assert state(read(ctx)) == state(before)
    ctx.wrap_molecules()
    assert state(read(ctx)) == state(expected("water13", "mixed"))
    # a new table on a live handle: the device tables follow
    ctx.set_molecules(case("water13-merged")[1])
    load(ctx, before)
    f = ctx.frame(wrap=True, skip_drude=True).cpu().numpy()
    assert f.tobytes() == expected_frame("water13-merged", "mixed", WRAP | SKIP_DRUDE, 1.0).tobytes()
    ctx.wrap_molecules()
    assert state(read(ctx)) == state(expected("water13-merged", "mixed"))
    ctx.set_molecules(None)
    load(ctx, before)
    assert ctx.frame(wrap=True, skip_drude=True).cpu().numpy().tobytes() == expected_frame("water13", "mixed", WRAP | SKIP_DRUDE, 1.0).tobytes()
    ctx.wrap_molecules()
    assert state(read(ctx)) == state(expected("water13", "mixed"))
    ctx.close()


def test_dualnh_without_resid_writes_plain_frames():
    from test_scale_positions import _WithoutResid
    s = synth.water_box(13)[0]
    ctx = HipContext(_WithoutResid(s), integ(), mode="dualNH", precision="mixed")
    before = start("water13", "mixed")
    load(ctx, before)
    ctx.setPeriodicBoxVectors(*BOX)
    for skip in (False, True):
        f = ctx.frame(skip_drude=skip, unit=10.0).cpu().numpy()
        assert f.tobytes() == frame_of(before, None, s.pair_drude, None, SKIP_DRUDE if skip else 0, 10.0, "mixed").tobytes()
    assert status_of(ctx.wrap_molecules) == _lib.ERR_STATE and "tgnh_set_molecules first" in ctx.lib.tgnh_last_error().decode()
    assert status_of(lambda: ctx.frame(wrap=True)) == _lib.ERR_STATE
    assert state(read(ctx)) == state(before)
    ctx.set_molecules(s.resid)
    ctx.wrap_molecules()
    assert state(read(ctx)) == state(expected("water13", "mixed"))
    ctx.close()


@pytest.mark.parametrize("precision", ["double", "mixed", "single"])
def test_a_handle_without_pairs(precision):
    s = synth.DrudeSystem(mass=np.array([12.0, 1.0, 0.0]), pair_drude=np.zeros(0, np.int32), pair_parent=np.zeros(0, np.int32),
                          resid=np.zeros(3, np.int32), positions=np.arange(9.0).reshape(3, 3) / 7.0, velocities=np.zeros((3, 3)))
    ctx = HipContext(s, integ(), precision=precision)
    before = arrays(s.positions + WSHIFT, [0.1, -0.2, 0.3], precision)
    load(ctx, before)
    ctx.setPeriodicBoxVectors(*BOX)
    assert ctx.frame_count() == ctx.frame_count(skip_drude=True) == 3
    for flags in (WRAP | SKIP_DRUDE, SKIP_DRUDE, 0):
        f = ctx.frame(wrap=bool(flags & WRAP), skip_drude=bool(flags & SKIP_DRUDE), unit=10.0).cpu().numpy()
        assert f.tobytes() == frame_of(before, s.resid, [], BOX, flags, 10.0, precision).tobytes()
    ctx.wrap_molecules()
    want = wrapped(before, s.resid, BOX, precision)
    assert state(read(ctx)) == state(want) != state(before)
    ctx.close()
