"""CPU tests of tgnh_get_drude_statistics: the yardstick and the argument checks.

`stats` restates include/drude_tgnh.h's formulas in numpy -- per pair in fp64 from the positions as the arrays hold them, the
float / float-plus-correction split of mixed precision done the way HipContext.setPositions does it -- and is what
tests/test_drude_stats_gpu.py holds the kernel against.  `configure` and `conditions` build and vet that file's cases; they live
here so that the choice of seed is checked without a GPU."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator, DrudeStatistics, HostTopology
from openmm_drudenose_amd.system import DrudeSystem

BINS = _lib.DRUDE_HIST_BINS


def stored(positions, charges, precision):
    """coordinates [N, 3] and charges [N] in fp64, as the kernel reads them off posq (+ posq_correction)"""
    p = np.ascontiguousarray(positions, np.float64)
    q = np.ascontiguousarray(charges, np.float64)
    if precision == "double":
        return p, q
    hi = p.astype(np.float32)
    x = hi.astype(np.float64)
    if precision == "mixed":
        x = x + (p - hi.astype(np.float64)).astype(np.float32).astype(np.float64)
    return x, q.astype(np.float32).astype(np.float64)


def stats(system, positions, charges, precision, threshold, hist_max):
    """include/drude_tgnh.h, restated.  Besides the fields of tgnh_drude_stats: the per-pair d and d2 (pair order), and the sums
    of the absolute values of what sum_d2 and dipole add up (the tolerance of a sum in another order)."""
    x, q = stored(positions, charges, precision)
    pd, pp = np.asarray(system.pair_drude, np.int64), np.asarray(system.pair_parent, np.int64)
    P = len(pd)
    out = SimpleNamespace(pairs=P, over=0, max_distance=0.0, worst_particle=-1, sum_d2=0.0, dipole=np.zeros(3),
                          hist=np.zeros(BINS + 1, np.int64), d=np.zeros(0), d2=np.zeros(0), abs_sum_d2=0.0, abs_dipole=np.zeros(3))
    if P == 0:
        return out
    delta = x[pd] - x[pp]
    dx, dy, dz = delta[:, 0], delta[:, 1], delta[:, 2]
    d2 = dx * dx + dy * dy + dz * dz                          # (numpy rounds each product and each sum: no fused multiply-add)
    d = np.sqrt(d2)
    out.d, out.d2 = d, d2
    out.over = int((d2 > threshold * threshold).sum())
    top = d2.max()
    out.max_distance = float(np.sqrt(top))
    out.worst_particle = int(pd[d2 == top].min())             # ties: the lowest slot index
    out.sum_d2, out.abs_sum_d2 = float(d2.sum()), float(d2.sum())
    terms = q[pd][:, None] * delta
    out.dipole, out.abs_dipole = terms.sum(0), np.abs(terms).sum(0)
    if hist_max > 0:
        t = d * BINS / hist_max
        k = np.where(t >= BINS, BINS, np.floor(np.minimum(t, BINS))).astype(np.int64)
        out.hist = np.bincount(k, minlength=BINS + 1).astype(np.int64)
    return out


# ---- the cases of tests/test_drude_stats_gpu.py ----
THRESHOLD, HIST_MAX = 0.01, 0.012         # nm: of the sigma = 0.002 nm displacements about 1 in 10^5 lies beyond either; the boosted pairs do
SEED = 20240607
BOOST = (4.0, 7.0, 11.0)                  # factors on the displacements of the first, middle and last pair


def configure(system, seed=SEED):
    """positions and charges of a case: every Drude particle displaced from its parent by a seeded Gaussian, sigma = 0.002 nm per
    axis (SURVEY 8d's configs), three hand-picked pairs' displacements multiplied so that pairs lie beyond the threshold and
    beyond the histogram; charges -1 .. -2 e on the Drude particles, anything on the others (only the former may enter)."""
    rng = np.random.default_rng(seed)
    P = system.num_pairs
    disp = rng.normal(0.0, 0.002, (P, 3))
    picked = sorted({0, P // 2, P - 1})
    for k, f in zip(picked, BOOST):
        disp[k] *= f
    pos = np.array(system.positions, np.float64)
    pos[system.pair_drude] = pos[system.pair_parent] + disp
    q = rng.uniform(-3.0, 3.0, system.num_particles)
    q[system.pair_drude] = rng.uniform(-2.0, -1.0, P)
    return pos, q


def conditions(ref, threshold, hist_max):
    """what makes the integer fields comparable exactly: no pair's d within a relative 1e-9 of the threshold or of a bin edge,
    and the two largest d2 apart.  Over every pair."""
    d = ref.d
    assert (np.abs(d - threshold) > 1e-9 * threshold).all()
    if hist_max > 0:
        edges = np.arange(1, BINS + 1) * hist_max / BINS
        assert (np.abs(d[:, None] - edges[None, :]) > 1e-9 * edges[None, :]).all()
    if len(d) > 1:
        top = np.sort(ref.d2)[-2:]
        assert top[1] > top[0]


def gpu_cases():
    from test_gather_gpu import drudes_at_the_end              # (its builder, as that file uses it)
    return {"pair+normal+massless": (synth.pair_normal_massless, ("double", "mixed", "single")),
            "nacl": (synth.nacl, ("double", "mixed", "single")),
            "water216": (lambda: synth.water_box(216), ("double", "mixed", "single")),
            "drudes-at-the-end": (lambda: drudes_at_the_end(300), ("mixed",)),
            # INDEX_GRID_CAP x work-group size = 1024 x 256 = 262 144 slots in one trip of the grid-stride loop: 262 500 slots,
            # so the first 356 threads make two
            "water52500": (lambda: synth.water_box(52_500), ("mixed",))}


def integ(hardwall=0.0):
    it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 3, True, True)
    it.setMaxDrudeDistance(hardwall)
    return it


# ---- the yardstick's own checks ----
def three_pairs():
    """parents at slots 0, 2, 5, Drude particles at 1, 4, 3 (the pair list in another order than the slots), one loose particle;
    distances 0.25 along x, 0.5 along y, 1.0 along z: exact in every precision"""
    pos = np.zeros((7, 3))
    pos[[0, 2, 5, 6]] = [[1.0, 2.0, 3.0], [-2.0, 0.5, 0.25], [4.0, 4.0, -8.0], [9.0, 9.0, 9.0]]
    pos[1] = pos[0] + [0.25, 0.0, 0.0]
    pos[4] = pos[2] + [0.0, -0.5, 0.0]
    pos[3] = pos[5] + [0.0, 0.0, 1.0]
    s = DrudeSystem(mass=np.array([12.0, 0.4, 12.0, 0.4, 0.4, 12.0, 1.0]), pair_drude=np.array([4, 1, 3]), pair_parent=np.array([2, 0, 5]),
                    resid=np.array([0, 0, 1, 2, 1, 2, 3]), positions=pos)
    q = np.array([7.0, -1.0, 5.0, -1.5, -2.0, 3.0, 11.0])
    return s, pos, q


@pytest.mark.parametrize("precision", ["double", "mixed", "single"])
def test_three_pairs_by_hand(precision):
    s, pos, q = three_pairs()
    r = stats(s, pos, q, precision, 0.4, 1.0)
    assert (r.pairs, r.over, r.worst_particle) == (3, 2, 3)
    assert r.max_distance == 1.0 and r.sum_d2 == 0.0625 + 0.25 + 1.0
    want = np.zeros(BINS + 1, np.int64)
    want[8] = want[16] = want[BINS] = 1                       # floor(0.25 x 32), floor(0.5 x 32), d >= hist_max
    assert np.array_equal(r.hist, want)
    assert np.array_equal(r.dipole, [-1.0 * 0.25, -2.0 * -0.5, -1.5 * 1.0])
    assert np.array_equal(r.abs_dipole, [0.25, 1.0, 1.5])
    off = stats(s, pos, q, precision, 2.0, 0.0)               # hist_max == 0: no histogram
    assert off.over == 0 and not off.hist.any()
    conditions(r, 0.4, 0.7)
    with pytest.raises(AssertionError):
        conditions(r, 0.25, 1.0)                              # a pair on the threshold
    with pytest.raises(AssertionError):
        conditions(r, 0.4, 1.0)                               # ... and on a bin edge


def test_a_tie_goes_to_the_lowest_slot():
    s, pos, q = three_pairs()
    pos[4] = pos[2] + [0.0, 0.0, -1.0]                        # |d| = 1 twice: Drude slots 3 and 4, slot 4 first in the pair list
    r = stats(s, pos, q, "mixed", 0.4, 1.0)
    assert r.worst_particle == 3 and r.max_distance == 1.0 and r.hist[BINS] == 2
    with pytest.raises(AssertionError):
        conditions(r, 0.4, 0.0)                               # (such a system is no case for an exact comparison)


def test_no_pair():
    s = DrudeSystem(mass=np.ones(3), pair_drude=np.zeros(0, np.int32), pair_parent=np.zeros(0, np.int32), resid=np.zeros(3, np.int32),
                    positions=np.ones((3, 3)))
    r = stats(s, s.positions, np.ones(3), "mixed", 0.0, 1.0)
    assert (r.pairs, r.over, r.worst_particle, r.max_distance, r.sum_d2) == (0, 0, -1, 0.0, 0.0)
    assert not r.dipole.any() and not r.hist.any()


def test_mixed_precision_keeps_what_single_drops():
    s, _, _ = synth.water_box(8)
    pos, q = configure(s)
    dd, dm, ds = (stats(s, pos, q, p, THRESHOLD, HIST_MAX).d for p in ("double", "mixed", "single"))
    assert np.abs(dm - dd).max() < 1e-14 and 1e-10 < np.abs(ds - dd).max() < 1e-6


def test_the_cases_of_the_gpu_tests_are_comparable_exactly():
    """The seed is chosen for this: the yardstick alone says that no pair sits on the threshold or on a bin edge and that the
    largest distance is the largest alone, in every case and precision the GPU tests run; and every case has pairs beyond the
    threshold and beyond the histogram."""
    for name, (build, precisions) in gpu_cases().items():
        s = build()[0]
        pos, q = configure(s)
        for precision in precisions:
            r = stats(s, pos, q, precision, THRESHOLD, HIST_MAX)
            conditions(r, THRESHOLD, HIST_MAX)
            assert r.over > 0 and r.hist[BINS] > 0 and r.hist.sum() == r.pairs == s.num_pairs, (name, precision)
    assert gpu_cases()["water52500"][0]()[0].num_particles > 1024 * 256


# ---- the entry point's argument checks (a host-only handle, no GPU) ----
def new_stats(size=None):
    st = _lib.TgnhDrudeStats()
    st.struct_size = C.sizeof(st) if size is None else size
    return st


def test_the_binding_has_the_headers_layout():
    assert C.sizeof(_lib.TgnhDrudeStats) == 4 + 4 + 8 + 8 + 8 + 8 + 24 + 8 * (BINS + 1)
    assert _lib.TgnhDrudeStats.hist.offset == 64 and _lib.TgnhDrudeStats.dipole.offset == 40


def test_argument_checks_through_a_host_only_handle():
    lib = _lib.load()
    s, _, _ = synth.nacl()
    top = HostTopology(s, integ(), mode="TGNH")
    call = lib.tgnh_get_drude_statistics
    st = new_stats()
    assert call(None, 0.02, 0.0, None, C.byref(st)) == _lib.ERR_ARG                 # a null handle
    assert call(top.h, 0.02, 0.0, None, None) == _lib.ERR_ARG                       # a null out
    for size in (0, C.sizeof(st) - 8, C.sizeof(st) + 8):
        bad = new_stats(size)
        assert call(top.h, 0.02, 0.0, None, C.byref(bad)) == _lib.ERR_ARG, size
        assert b"size" in lib.tgnh_last_error()
    for thr, hmax in ((-1e-9, 0.0), (np.nan, 0.0), (np.inf, 0.0), (0.02, -1.0), (0.02, np.nan), (0.02, np.inf)):
        assert call(top.h, thr, hmax, None, C.byref(st)) == _lib.ERR_ARG, (thr, hmax)
    before = bytes(st)
    assert call(top.h, 0.02, 0.05, None, C.byref(st)) == _lib.ERR_STATE             # legal values: the refusal is the handle's
    assert call(top.h, 0.0, 0.0, None, C.byref(st)) == _lib.ERR_STATE
    assert bytes(st) == before                                                      # nothing of *out was written
    top.close()


def test_the_result_object_is_read_only():
    st = new_stats()
    st.pairs, st.over, st.worst_particle, st.max_distance, st.sum_d2 = 4, 1, 7, 0.03, 4 * 0.01 ** 2
    st.dipole[:] = [1.0, 2.0, 3.0]
    st.hist[BINS] = 1
    r = DrudeStatistics(st, 0.02, 0.032)
    assert (r.pairs, r.over, r.worst_particle, r.max_distance) == (4, 1, 7, 0.03)
    assert r.rms_distance == pytest.approx(0.01, rel=1e-15) and r.induced_dipole.tolist() == [1.0, 2.0, 3.0]
    assert r.hist.dtype == np.int64 and r.hist.shape == (BINS + 1,) and r.hist[BINS] == 1
    assert r.hist_edges.shape == (BINS + 1,) and r.hist_edges[1] == pytest.approx(0.001) and r.hist_edges[-1] == 0.032
    assert DrudeStatistics(st, 0.02, 0.0).hist_edges is None
    with pytest.raises(AttributeError):
        r.pairs = 5
    with pytest.raises(ValueError):
        r.hist[0] = 1
    assert r.raw == bytes(st)
