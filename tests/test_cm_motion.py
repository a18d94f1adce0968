"""CPU tests of the centre-of-mass calls (tgnh_get_momentum, tgnh_shift_velocities, tgnh_remove_cm_motion,
tgnh_set_cm_motion_removal): the yardstick and the argument checks.

`momentum` and `removed` restate include/drude_tgnh.h's formulas in numpy -- per slot in fp64 from velm as the array holds it,
m = 1.0 / (double)w, every product rounded on its own, the terms added one after the other in slot order (np.cumsum: a plain
ordered sum, neither pairwise nor compensated), the shifted velocity rounded once to velm's type -- and are what
tests/test_cm_motion_gpu.py holds the kernels against."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator, HostTopology, Momentum, FLAG_DEFER_SCALE

STORE = {"single": np.float32, "mixed": np.float64, "double": np.float64}


def ordered_sum(terms):
    """terms [n] or [n, k] added in index order, each partial sum rounded (fp64)"""
    return np.cumsum(terms, axis=0, dtype=np.float64)[-1] if len(terms) else np.zeros(terms.shape[1:])


def momentum(velm, precision):
    """include/drude_tgnh.h, restated.  velm [N, 4] in its stored type.  Besides the fields of tgnh_momentum: velocity = P / M, the
    sums of the absolute values of what mass and momentum add up (the tolerance of a sum in another order), and the mask of the
    massive slots."""
    velm = np.asarray(velm)
    assert velm.dtype == STORE[precision] and velm.ndim == 2 and velm.shape[1] == 4
    w = velm[:, 3].astype(np.float64)
    massive = w != 0
    m = 1.0 / w[massive]
    terms = m[:, None] * velm[massive, :3].astype(np.float64)      # (numpy rounds each product: no fused multiply-add)
    out = SimpleNamespace(massive=int(massive.sum()), mask=massive, m=m)
    out.mass, out.abs_mass = float(ordered_sum(m)), float(ordered_sum(np.abs(m)))
    out.momentum, out.abs_momentum = ordered_sum(terms), ordered_sum(np.abs(terms))
    out.velocity = out.momentum / out.mass if out.mass != 0 else np.zeros(3)
    return out


def shifted(velm, precision, dv):
    """v' = (type of velm)((double)v - dv) on every massive slot; everything else bit for bit"""
    velm = np.asarray(velm)
    out = velm.copy()
    massive = velm[:, 3] != 0
    out[massive, :3] = (velm[massive, :3].astype(np.float64) - np.asarray(dv, np.float64)).astype(STORE[precision])
    return out


def removed(velm, precision):
    mom = momentum(velm, precision)
    return shifted(velm, precision, mom.velocity) if mom.mass != 0 else np.array(velm, copy=True)


def integ(chains=3):
    return DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, chains, True, True)


# ---- the yardstick's own checks ----
def by_hand():
    """masses 2, 0.5, none, 4 (w exact in every type); every product and sum below is exact in fp32"""
    return np.array([[1.0, -2.0, 0.5, 0.5],
                     [4.0, 8.0, -16.0, 2.0],
                     [7.0, 7.0, 7.0, 0.0],
                     [0.25, 0.0, -1.0, 0.25]])


@pytest.mark.parametrize("precision", ["double", "mixed", "single"])
def test_by_hand(precision):
    velm = by_hand().astype(STORE[precision])
    r = momentum(velm, precision)
    assert (r.massive, r.mass, r.abs_mass) == (3, 6.5, 6.5)
    assert r.momentum.tolist() == [2.0 + 2.0 + 1.0, -4.0 + 4.0 + 0.0, 1.0 - 8.0 - 4.0]
    assert r.abs_momentum.tolist() == [5.0, 8.0, 13.0]
    assert r.velocity.tolist() == [5.0 / 6.5, 0.0, -11.0 / 6.5]
    out = removed(velm, precision)
    assert out.dtype == velm.dtype
    assert out[:, 3].tobytes() == velm[:, 3].tobytes() and out[2].tobytes() == velm[2].tobytes()      # w; the massless slot
    want = (velm[[0, 1, 3], :3].astype(np.float64) - r.velocity).astype(velm.dtype)
    assert np.array_equal(out[[0, 1, 3], :3], want)
    left = momentum(out, precision)
    u = 2.0 ** -24 if precision == "single" else 2.0 ** -53
    # what is left: every stored v' is off by <= u |v'| <= u (|v| + |v_cm|), and the three-term fp64 sums by 3 x 2^-52 of the same
    reach = r.abs_momentum + np.abs(r.velocity) * r.abs_mass
    assert (np.abs(left.momentum) <= (u + 3 * 2.0 ** -52) * reach).all()
    assert np.array_equal(shifted(velm, precision, [0.0, 0.0, 0.0]), velm)


def test_the_sum_is_the_plain_ordered_one():
    """1 + 2^-53 + 2^-53 + ...: the ordered sum drops every small term, a pairwise or compensated one would not"""
    velm = np.zeros((1025, 4))
    velm[:, 3] = 1.0 / 2.0 ** -53
    velm[0, 3] = 1.0
    r = momentum(velm, "double")
    assert r.mass == 1.0 and r.abs_mass == 1.0 and r.massive == 1025
    assert float(np.sum(1.0 / velm[:, 3])) > 1.0


def test_no_mass():
    velm = np.ones((3, 4), np.float32)
    velm[:, 3] = 0
    r = momentum(velm, "single")
    assert (r.massive, r.mass) == (0, 0.0) and not r.momentum.any() and not r.velocity.any()
    assert removed(velm, "single").tobytes() == velm.tobytes()


# ---- the binding and the entry points' argument checks (host-only handles, no GPU) ----
def new_momentum(size=None):
    st = _lib.TgnhMomentum()
    st.struct_size = C.sizeof(st) if size is None else size
    return st


def test_the_binding_has_the_headers_layout():
    assert C.sizeof(_lib.TgnhMomentum) == 4 + 4 + 8 + 8 + 24
    T = _lib.TgnhMomentum
    assert (T.struct_size.offset, T.reserved.offset, T.massive.offset, T.mass.offset, T.momentum.offset) == (0, 4, 8, 16, 24)


def test_argument_checks_through_a_host_only_handle():
    lib = _lib.load()
    s, _, _ = synth.nacl()
    top = HostTopology(s, integ(), mode="TGNH")
    dv = (C.c_double * 3)(0.1, 0.2, 0.3)
    st = new_momentum()
    # a null handle
    assert lib.tgnh_get_momentum(None, None, C.byref(st)) == _lib.ERR_ARG
    assert lib.tgnh_shift_velocities(None, dv, None) == _lib.ERR_ARG
    assert lib.tgnh_remove_cm_motion(None, None) == _lib.ERR_ARG
    assert lib.tgnh_set_cm_motion_removal(None, 1) == _lib.ERR_ARG
    # arguments
    assert lib.tgnh_get_momentum(top.h, None, None) == _lib.ERR_ARG
    for size in (0, C.sizeof(st) - 8, C.sizeof(st) + 8):
        bad = new_momentum(size)
        kept = bytes(bad)
        assert lib.tgnh_get_momentum(top.h, None, C.byref(bad)) == _lib.ERR_ARG, size
        assert b"size" in lib.tgnh_last_error() and bytes(bad) == kept
    assert lib.tgnh_shift_velocities(top.h, None, None) == _lib.ERR_ARG
    for k in range(3):
        for v in (np.nan, np.inf, -np.inf):
            odd = (C.c_double * 3)(0.0, 0.0, 0.0)
            odd[k] = v
            assert lib.tgnh_shift_velocities(top.h, odd, None) == _lib.ERR_ARG, (k, v)
    assert lib.tgnh_set_cm_motion_removal(top.h, -1) == _lib.ERR_ARG
    # legal arguments: the refusal is the handle's (device -1: nothing launches)
    before = bytes(st)
    assert lib.tgnh_get_momentum(top.h, None, C.byref(st)) == _lib.ERR_STATE
    assert bytes(st) == before                                                      # nothing of *out was written
    assert lib.tgnh_shift_velocities(top.h, dv, None) == _lib.ERR_STATE
    assert lib.tgnh_remove_cm_motion(top.h, None) == _lib.ERR_STATE
    # the setter only takes note
    for every in (0, 1, 3, 0):
        assert lib.tgnh_set_cm_motion_removal(top.h, every) == _lib.TGNH_OK
    top.close()


def test_the_setter_is_refused_on_a_deferred_handle():
    lib = _lib.load()
    s, _, _ = synth.nacl()
    top = HostTopology(s, integ(), mode="TGNH", flags=FLAG_DEFER_SCALE)
    assert lib.tgnh_set_cm_motion_removal(top.h, 1) == _lib.ERR_UNSUPPORTED
    assert b"DEFER_SCALE" in lib.tgnh_last_error()
    assert lib.tgnh_set_cm_motion_removal(top.h, 0) == _lib.TGNH_OK                 # off is what it is already
    assert lib.tgnh_set_cm_motion_removal(top.h, -1) == _lib.ERR_ARG
    top.close()


def test_the_result_object_is_read_only():
    st = new_momentum()
    st.massive, st.mass = 3, 6.5
    st.momentum[:] = [5.0, 0.0, -11.0]
    r = Momentum(st)
    assert (r.massive, r.mass) == (3, 6.5) and r.momentum.tolist() == [5.0, 0.0, -11.0]
    assert r.velocity.tolist() == [5.0 / 6.5, 0.0, -11.0 / 6.5] and r.raw == bytes(st)
    with pytest.raises(AttributeError):
        r.mass = 1.0
    with pytest.raises(ValueError):
        r.momentum[0] = 1.0
    empty = Momentum(new_momentum())
    assert empty.mass == 0.0 and not empty.velocity.any()
