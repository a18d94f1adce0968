"""CPU tests of the molecule table (tgnh_set_molecules, tgnh_get_num_molecules, tgnh_get_molecules), of the argument checks of
tgnh_scale_positions / tgnh_restore_positions, and of barostat.MonteCarloBarostat: the yardstick and everything a host-only handle
answers.

`scaled` restates include/drude_tgnh.h's formulas in numpy -- per component in fp64 from the arrays as they are stored, x(i) = posq
(+ posq_correction in mixed precision), a molecule's sum taken member by member in ascending slot order from the first member's
value (vectorised over the molecules, sequential over the member rank k: every partial sum rounded, neither pairwise nor
compensated), c = S / n, d = c (scale - 1), x' = x + d, each rounded on its own (numpy fuses nothing), stored as the header says
-- and is what tests/test_scale_positions_gpu.py holds the kernels against."""
import ctypes as C
import math

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.barostat import MonteCarloBarostat, AVOGADRO
from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator, HostTopology, TgnhError, FLAG_GATHER

REAL = {"single": np.float32, "mixed": np.float32, "double": np.float64}
SHIFT = np.array([3.1, -2.7, 0.4])              # nm: centroids far from zero
ANISO = (1.013, 0.991, 1.0007)


def renumbered(labels):
    """labels -> 0..M-1 in order of first appearance"""
    labels = np.asarray(labels)
    _, first, inv = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.int32)


def coordinates(posq, corr):
    x = np.asarray(posq)[:, :3].astype(np.float64)
    return x if corr is None else x + np.asarray(corr)[:, :3].astype(np.float64)


def stored(x, precision):
    """positions [N, 3] fp64 -> (posq xyz, correction xyz or None) in the stored types, as setPositions and the kernels split them"""
    if precision == "double":
        return x.copy(), None
    hi = x.astype(np.float32)
    return hi, ((x - hi.astype(np.float64)).astype(np.float32) if precision == "mixed" else None)


def centroids(x, mol):
    """-> (S [M, 3], c [M, 3], n [M], sum|x| [M, 3]); S in the header's order"""
    order = np.argsort(mol, kind="stable")                 # the slots by molecule, ascending within one
    n = np.bincount(mol)
    start = np.r_[0, np.cumsum(n)[:-1]]
    S = x[order[start]].copy()
    A = np.abs(S)
    for k in range(1, int(n.max())):
        sel = np.flatnonzero(n > k)
        term = x[order[start[sel] + k]]
        S[sel] = S[sel] + term
        A[sel] = A[sel] + np.abs(term)
    return S, S / n[:, None].astype(np.float64), n, A


def scaled(pos_arrays, labels, scale, precision):
    """include/drude_tgnh.h, tgnh_scale_positions, restated.  pos_arrays = (posq [N, 4], posq_correction [N, 4] or None) in their stored
    types -> the same pair after the move; w of both bit for bit."""
    posq, corr = pos_arrays
    posq = np.asarray(posq)
    assert posq.dtype == REAL[precision] and posq.shape[1] == 4 and (corr is not None) == (precision == "mixed")
    mol = renumbered(labels)
    x = coordinates(posq, corr)
    _, c, _, _ = centroids(x, mol)
    sm1 = np.broadcast_to(np.asarray(scale, np.float64), (3,)) - 1.0
    xn = x + (c * sm1)[mol]
    hi, lo = stored(xn, precision)
    out, out_corr = posq.copy(), None
    out[:, :3] = hi
    if corr is not None:
        out_corr = np.asarray(corr).copy()
        out_corr[:, :3] = lo
    return out, out_corr


def arrays(positions, charges, precision):
    """(posq, corr) of these positions [N, 3] and charges [N] in the stored types; the correction's w is set to a pattern of its own"""
    hi, lo = stored(np.asarray(positions, np.float64), precision)
    posq = np.zeros((len(hi), 4), REAL[precision])
    posq[:, :3], posq[:, 3] = hi, charges
    corr = None
    if lo is not None:
        corr = np.zeros((len(hi), 4), np.float32)
        corr[:, :3], corr[:, 3] = lo, np.arange(len(hi)) % 7 - 3.0
    return posq, corr


def integ(chains=3):
    return DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, chains, True, True)


# ---- the yardstick's own checks ----
def test_the_yardstick_against_a_plain_loop():
    """every centroid of synth.nacl() within n 2^-52 sum|x| / n of a plain Python loop in long double: (n - 1) roundings of 2^-53
    sum|x| in the sum, one more in the division"""
    s, _, _ = synth.nacl()
    x = s.positions + SHIFT
    mol = renumbered(s.resid)
    S, c, n, A = centroids(x, mol)
    assert len(n) == 512 and set(n.tolist()) == {5, 2}
    for m in range(len(n)):
        acc = np.zeros(3, np.longdouble)
        for i in np.flatnonzero(mol == m):
            acc = acc + x[i].astype(np.longdouble)
        exact = acc / np.longdouble(n[m])
        assert (np.abs(c[m].astype(np.longdouble) - exact) <= 2.0 ** -52 * A[m]).all(), m
    # ... and the move itself: x' - x is the molecule's d, rounded once
    out, _ = scaled(arrays(x, np.zeros(len(x)), "double"), s.resid, ANISO, "double")
    d = (c * (np.array(ANISO) - 1.0))[mol]
    assert np.array_equal(out[:, :3], x + d)


@pytest.mark.parametrize("precision", ["double", "mixed", "single"])
def test_by_hand(precision):
    """members that share a coordinate: S = 3 x 2, c = 2, d = 2 x 0.5 = 1, x' = 3, every step exact in every type"""
    x = np.array([[2.0, 1.0, -4.0], [8.0, 8.0, 8.0], [2.0, 3.0, -4.0], [2.0, 5.0, -4.0]])
    labels = [7, -3, 7, 7]                                 # one molecule in two runs, one of a single slot
    posq, corr = arrays(x, [0.5, -1.0, 0.25, 2.0], precision)
    out, out_corr = scaled((posq, corr), labels, 1.5, precision)
    assert out.dtype == posq.dtype and out[:, 3].tobytes() == posq[:, 3].tobytes()
    assert out[:, :3].tolist() == [[3.0, 2.5, -6.0], [12.0, 12.0, 12.0], [3.0, 4.5, -6.0], [3.0, 6.5, -6.0]]
    if corr is not None:
        assert out_corr[:, 3].tobytes() == corr[:, 3].tobytes() and not out_corr[:, :3].any()
    same, same_corr = scaled((posq, corr), labels, (1.0, 1.0, 1.0), precision)
    assert same.tobytes() == posq.tobytes() and (corr is None or same_corr.tobytes() == corr.tobytes())


def test_the_sum_is_the_plain_ordered_one():
    """1 + 2^-53 + 2^-53 + ...: the ordered sum drops every small term, a pairwise one would not"""
    x = np.full((40, 3), 2.0 ** -53)
    x[0] = 1.0
    S, c, n, _ = centroids(x, np.zeros(40, np.int32))
    assert (S == 1.0).all() and n.tolist() == [40] and float(np.sum(x[:, 0])) > 1.0


def test_renumbering():
    assert renumbered([5, 5, -2, 9, -2, 5]).tolist() == [0, 0, 1, 2, 1, 0]


# ---- the molecule table through host-only handles ----
def table(top):
    return top.num_molecules(), top.molecules()


def test_the_default_table_is_the_residues():
    s, _, _ = synth.water_box(13)
    top = HostTopology(s, integ())
    m, mol = table(top)
    assert m == 13 and mol.tolist() == np.repeat(np.arange(13), 5).tolist()
    top.close()


def test_a_residue_in_two_runs_is_one_molecule():
    from helpers import drudes_at_the_end
    s, _, _ = drudes_at_the_end(300)
    top = HostTopology(s, integ())
    assert top.step_path()[0] == "gather"
    m, mol = table(top)
    assert m == 300 and np.array_equal(mol, renumbered(s.resid))
    assert np.array_equal(mol[s.pair_drude], mol[s.pair_parent])
    top.close()


def test_labels_are_renumbered_by_first_appearance():
    s, _, _ = synth.water_box(4)
    top = HostTopology(s, integ())
    labels = np.repeat([2 ** 31 - 1, -7, 2 ** 31 - 1, -2 ** 31], 5).astype(np.int32)
    top.set_molecules(labels)
    m, mol = table(top)
    assert m == 3 and mol.tolist() == np.repeat([0, 1, 0, 2], 5).tolist()
    top.set_molecules(None)                                 # back to the default
    assert table(top)[0] == 4
    with pytest.raises(TgnhError) as e:
        top.set_molecules(np.zeros(19, np.int32))
    assert e.value.status == _lib.ERR_ARG
    top.close()


def test_labels_that_split_a_pair_are_refused():
    s, _, _ = synth.water_box(4)
    top = HostTopology(s, integ())
    labels = np.repeat(np.arange(4), 5).astype(np.int32)
    k = 2
    labels[s.pair_drude[k]] = 99
    with pytest.raises(TgnhError) as e:
        top.set_molecules(labels)
    assert e.value.status == _lib.ERR_ARG
    assert f"pair {k} " in str(e.value) and str(int(s.pair_drude[k])) in str(e.value) and str(int(s.pair_parent[k])) in str(e.value)
    assert table(top)[0] == 4                               # the table in force is untouched
    top.close()


def test_a_resid_that_splits_a_pair_fails_as_the_default():
    s, _, _ = synth.water_box(4)
    resid = s.resid.copy()
    resid[s.pair_drude[1]] = 0 if resid[s.pair_drude[1]] else 1
    odd = synth.DrudeSystem(mass=s.mass, pair_drude=s.pair_drude, pair_parent=s.pair_parent, resid=resid, positions=s.positions,
                            velocities=s.velocities)
    top = HostTopology(odd, integ(), mode="dualNH")
    lib = top.lib
    n = C.c_int()
    assert lib.tgnh_get_num_molecules(top.h, C.byref(n)) == _lib.ERR_ARG and b"pair 1 " in lib.tgnh_last_error()
    assert lib.tgnh_set_molecules(top.h, None) == _lib.ERR_ARG
    top.close()


class _WithoutResid:
    """a DrudeSystem whose resid reaches tgnh_create as NULL"""
    class _Null:
        class ctypes:
            @staticmethod
            def data_as(_):
                return None
    resid = _Null()

    def __init__(self, s):
        self._s = s

    def __getattr__(self, name):
        return getattr(self._s, name)


def test_dualnh_without_resid_has_no_default():
    s, _, _ = synth.water_box(3)
    top = HostTopology(_WithoutResid(s), integ(), mode="dualNH")
    lib = top.lib
    n, out = C.c_int(), np.zeros(15, np.int32)
    assert lib.tgnh_get_num_molecules(top.h, C.byref(n)) == _lib.ERR_STATE and b"tgnh_set_molecules first" in lib.tgnh_last_error()
    assert lib.tgnh_get_molecules(top.h, out.ctypes.data_as(_lib.c_i32p)) == _lib.ERR_STATE
    assert lib.tgnh_set_molecules(top.h, None) == _lib.ERR_STATE
    top.set_molecules(s.resid)
    assert table(top)[0] == 3
    top.close()


def test_argument_checks_through_a_host_only_handle():
    lib = _lib.load()
    s, _, _ = synth.nacl()
    top = HostTopology(s, integ(), flags=FLAG_GATHER)
    ok = (C.c_double * 3)(*ANISO)
    n = C.c_int()
    assert lib.tgnh_set_molecules(None, None) == _lib.ERR_ARG
    assert lib.tgnh_get_num_molecules(None, C.byref(n)) == _lib.ERR_ARG and lib.tgnh_get_num_molecules(top.h, None) == _lib.ERR_ARG
    assert lib.tgnh_get_molecules(None, None) == _lib.ERR_ARG and lib.tgnh_get_molecules(top.h, None) == _lib.ERR_ARG
    assert lib.tgnh_scale_positions(None, ok, 0, None) == _lib.ERR_ARG and lib.tgnh_restore_positions(None, None) == _lib.ERR_ARG
    assert lib.tgnh_scale_positions(top.h, None, 0, None) == _lib.ERR_ARG
    for k in range(3):
        for v in (0.0, -1.0, -0.0, np.nan, np.inf, -np.inf):
            odd = (C.c_double * 3)(1.0, 1.0, 1.0)
            odd[k] = v
            assert lib.tgnh_scale_positions(top.h, odd, 1, None) == _lib.ERR_ARG, (k, v)
    # legal arguments: the refusal is the handle's (device -1: nothing launches)
    assert lib.tgnh_scale_positions(top.h, ok, 0, None) == _lib.ERR_STATE
    assert lib.tgnh_scale_positions(top.h, ok, 1, None) == _lib.ERR_STATE
    assert lib.tgnh_restore_positions(top.h, None) == _lib.ERR_STATE
    assert table(top)[0] == 512
    top.close()


def test_the_binding_declares_the_new_entry_points():
    S = _lib.SIGNATURES
    assert S["tgnh_set_molecules"] == (C.c_int, [C.c_void_p, _lib.c_i32p])
    assert S["tgnh_get_num_molecules"] == (C.c_int, [C.c_void_p, C.POINTER(C.c_int)])
    assert S["tgnh_get_molecules"] == (C.c_int, [C.c_void_p, _lib.c_i32p])
    assert S["tgnh_scale_positions"] == (C.c_int, [C.c_void_p, _lib.c_f64p, C.c_int, C.c_void_p])
    assert S["tgnh_restore_positions"] == (C.c_int, [C.c_void_p, C.c_void_p])
    header = open(_lib.os.path.join(_lib.HERE, "..", "include", "drude_tgnh.h")).read()
    for name in ("tgnh_set_molecules", "tgnh_get_num_molecules", "tgnh_get_molecules", "tgnh_scale_positions", "tgnh_restore_positions"):
        assert f"tgnh_status {name}(" in header


# ---- the barostat against a numpy stand-in ----
class StandIn:
    """The five context methods the barostat uses (and getPositions for the energy), on numpy arrays through `scaled`."""

    def __init__(self, positions, charges, labels, precision="double"):
        self.precision, self.labels = precision, renumbered(labels)
        self.posq, self.corr = arrays(positions, charges, precision)
        self.saved = None
        self.flushes = self.asked = 0

    def flush(self):
        self.flushes += 1

    def num_molecules(self):
        self.asked += 1
        return int(self.labels.max()) + 1

    def molecules(self):
        return self.labels

    def set_molecules(self, labels=None):
        self.labels = renumbered(labels)

    def scale_positions(self, scale, save=False):
        if save:
            self.saved = (self.posq.copy(), None if self.corr is None else self.corr.copy())
        self.posq, self.corr = scaled((self.posq, self.corr), self.labels, scale, self.precision)

    def restore_positions(self):
        self.posq, self.corr = self.saved[0].copy(), None if self.saved[1] is None else self.saved[1].copy()

    def getPositions(self):
        return coordinates(self.posq, self.corr)

    def state(self):
        return self.posq.tobytes() + (b"" if self.corr is None else self.corr.tobytes())


def centroid_energy(k, mol):
    """energy(context) = k sum |molecule centroid|^2, from getPositions() in numpy"""
    n = np.bincount(mol).astype(np.float64)

    def energy(ctx):
        x = ctx.getPositions()
        c = np.stack([np.bincount(mol, x[:, a]) for a in range(3)], 1) / n[:, None]
        return float(k * np.sum(c * c))
    return energy


def by_hand(updates, pressure_bar, temperature, seed, box, energy_of_scale, molecules):
    """One update after the other, written out.  energy_of_scale(None) is the potential energy as things stand, (s) with the trial
    move applied, (True / False) takes the decision.  -> (accepted [updates], volumeScale after each, final box edges)"""
    rng = np.random.default_rng(seed)
    P, kT = pressure_bar * AVOGADRO * 1e-25, synth.KB * temperature
    box = [float(b) for b in box]
    vscale = 0.01 * (box[0] * box[1] * box[2])
    acc, scales, tried, took = [], [], 0, 0
    trial = energy_of_scale
    for _ in range(updates):
        volume = box[0] * box[1] * box[2]
        u1, u2 = rng.random(), rng.random()
        e0 = trial(None)
        dv = vscale * 2 * (u1 - 0.5)
        s = ((volume + dv) / volume) ** (1.0 / 3.0)
        e1 = trial(s)
        w = e1 - e0 + P * dv - molecules * kT * math.log((volume + dv) / volume)
        ok = not (w > 0 and u2 > math.exp(-w / kT))
        trial(ok)
        if ok:
            box, volume = [b * s for b in box], volume + dv
        tried, took = tried + 1, took + ok
        if tried == 10:
            if took < 2.5:
                vscale = vscale / 1.1
            elif took > 7.5:
                vscale = min(vscale * 1.1, volume * 0.3)
            tried = took = 0
        acc.append(ok)
        scales.append(vscale)
    return acc, scales, box


def barostat_case(k, precision="double", n_water=27):
    """the system, labels and energy both files run the barostat on"""
    s, _, _ = synth.water_box(n_water)
    return s, renumbered(s.resid), s.positions + SHIFT, centroid_energy(k, renumbered(s.resid))


def run_barostat(ctx, energy, updates, seed, box):
    baro = MonteCarloBarostat(1.0, 300.0, frequency=25, seed=seed)
    acc, scales, states = [], [], []
    for _ in range(updates):
        before = ctx.state() if hasattr(ctx, "state") else None
        box, ok = baro.update(ctx, box, energy)
        if before is not None and not ok:
            assert ctx.state() == before                    # a rejected move: bit for bit
        acc.append(ok)
        scales.append(baro.volume_scale)
    return acc, scales, box, baro


BOX = np.array([4.5, 4.4, 4.6])


@pytest.mark.parametrize("k", [0.05, 2.0])
def test_the_barostat_against_a_straight_line_restatement(k):
    s, mol, x, energy = barostat_case(k)
    ctx = StandIn(x, np.zeros(len(x)), s.resid)
    acc, scales, box, baro = run_barostat(ctx, energy, 40, 11, BOX)
    assert ctx.flushes == 40 and ctx.asked == 40            # M comes from num_molecules(), the move is flushed for
    # the restatement keeps its own copy of the arrays and moves it with `scaled`, one trial at a time
    own = {"now": arrays(x, np.zeros(len(x)), "double"), "trial": None}

    def trial(what):
        if what is None:                                    # E0
            return energy(_Positions(own["now"]))
        if isinstance(what, (bool, np.bool_)):                # the decision
            if what:
                own["now"] = own["trial"]
            return None
        own["trial"] = scaled(own["now"], mol, what, "double")
        return energy(_Positions(own["trial"]))
    want_acc, want_scales, want_box = by_hand(40, 1.0, 300.0, 11, BOX, trial, 27)
    assert acc == want_acc and scales == want_scales and box.tolist() == want_box
    assert ctx.state() == own["now"][0].tobytes()
    assert scales[0] == 0.01 * float(np.prod(BOX))
    if k < 1:                                               # a soft potential: most moves are accepted and the step grows
        assert sum(acc) > 30 and scales[-1] > scales[0]
    else:                                                   # a stiff one: both outcomes
        assert True in acc and False in acc
    assert baro.total_attempted == 40 and baro.total_accepted == sum(acc)


class _Positions:
    def __init__(self, pos_arrays):
        self.pos_arrays = pos_arrays

    def getPositions(self):
        return coordinates(*self.pos_arrays)


def test_the_box_may_be_three_vectors():
    s, mol, x, energy = barostat_case(0.05)
    a = run_barostat(StandIn(x, np.zeros(len(x)), s.resid), energy, 5, 3, BOX)
    b = run_barostat(StandIn(x, np.zeros(len(x)), s.resid), energy, 5, 3, np.diag(BOX))
    assert a[0] == b[0] and np.allclose(np.diag(b[2]), a[2], rtol=1e-15, atol=0) and b[2].shape == (3, 3)
