"""Ewald summation on the library's NonbondedForce without a GPU (csrc/tgnh_ewald.*, tgnh_nonbonded.hip's Ewald instantiation;
include/drude_tgnh.h, EWALD SUMMATION, has the contract): an fp80 REFERENCE, an fp64 numpy TWIN that follows the header's sequence,
the states the GPU tests run (tests/test_ewald_gpu.py), and the checks that need no device.

 * THE REFERENCE restates the header in np.longdouble; erfc and erf come from mpmath at 34 digits, as a head and a tail.  It is held
   to: the Madelung energy of a 64-ion rock-salt cell (constant 1.7475645946331822) within 1e-14 of that energy -- at alpha rc = 6 and
   (pi kmax / (alpha L))^2 = 38.9 both truncations are below 1e-15 of it (erfc(6) = 2.2e-17, exp(-38.9) = 1.3e-17, over a thousand terms
   of alternating sign), and the constant itself carries 17 digits --; to the independence of the total from alpha at two converged
   settings, within 1e-14 of the sum of the eight energies' magnitudes by the same reasoning; and to central differences of its own
   energy per kind (direct, reciprocal, exclusion -- the last with a pair at r = 0 and a net charge), tests/test_nonbonded.py's method
   and its 1e-8 of the kind's largest force.
 * THE TWIN is the same code on float64: scipy.special.erfc / erf, numpy's exp, and for sincospi(2 t) the exact reduction
   u = 2 (t - rint(t)) followed by numpy's sin and cos of pi u.  C_m and S_m are added in slot order within parts of 4096 slots and the
   parts in order, the force's sum over the vectors in table order (np.cumsum is sequential), as the kernels do.  It cannot match the
   device bit for bit -- the math libraries differ -- and is not asked to.
 * MEASURED_MARGIN_EWALD.  The twin's largest deviation from the reference over every state of the GPU tests: for forces per slot and
   component relative to S_i, the sum of the absolute values of the terms the slot receives -- a pair's Coulomb and Lennard-Jones
   parts, the two terms of the exclusion correction and every (vector, slot) product of the reciprocal sum counted uncancelled --;
   for each of the eight energies relative to the sum of its terms' magnitudes.  test_the_margins prints every figure; the constant is
   the largest of them, one figure for forces and energies as tests/test_nonbonded.py's is.  GATE_EWALD = 16 x that, the project's
   factor: a device library that differs from numpy's by a few ulp a call is the twin's own order of error.  The force gate on the
   GPU is GATE_EWALD S_i plus 2^-33 per converted contribution of the slot (direct pairs and exclusion shares one by one, the
   reciprocal force once).
 * CONDITIONS on the states, asserted here: no pair within 1e-9 of the cutoff; an excluded pair at r = 0; a net charge; slots outside
   the box and at negative coordinates; more than one part of slots with a ragged last part; an M that is no multiple of 64; three
   different kmax on three different edges.
 * ewald_parameters on a water box at two tolerances: the RMS force error against a converged reference falls with the tolerance; the
   ratio error / tolerance is printed (a record: the rule is a heuristic).
 * every refusal of tgnh_set_nonbonded_ewald on a host-only handle with its status and text, nothing changed afterwards; the table
   class's new methods; NonbondedForces' three ways in."""
import ctypes as C
import math

import mpmath
import numpy as np
import pytest
import scipy.special

from openmm_drudenose_amd import _lib
from openmm_drudenose_amd.drudetgnhplugin import HostTopology, TgnhError
from openmm_drudenose_amd.forces import NonbondedForce, NonbondedForces
from openmm_drudenose_amd.system import DrudeSystem
from test_nonbonded import (PRECISIONS, FIXED, K, L, BOX_A, BOX_B, BOX_B_MORE, system_a, system_b, stored, integrator, excluded_matrix,
                            exception_terms, searched_pairs)

# test_the_margins_between_twin_and_reference prints the figures; when this was written the largest was the pair Lennard-Jones energy,
# 6.4e-14 (d = x(a) - x(b) rounded to fp64 where system B keeps molecules two box lengths outside the cell, times r^-12); forces 4.7e-14
MEASURED_MARGIN_EWALD = 7.0e-14
GATE_EWALD = 16 * MEASURED_MARGIN_EWALD
EW_PART = 4096
ENERGIES = ("pair Coulomb", "pair LJ", "exception Coulomb", "exception LJ", "reciprocal", "self", "background", "exclusion correction")
MADELUNG = 1.7475645946331822
_cache = {}
mpmath.mp.dps = 34


def _mp_to_l(v):
    hi = float(v)
    return L(hi) + L(float(v - hi))


def pi_of(dtype):
    return _mp_to_l(mpmath.pi) if dtype is L else np.float64(np.pi)


def _special(name, v, dtype):
    """erf or erfc of an array in dtype"""
    if dtype is np.float64:
        return getattr(scipy.special, name)(v)
    flat = np.asarray(v, L).ravel()
    uniq, inverse = np.unique(flat, return_inverse=True)
    fn = getattr(mpmath, name)
    out = np.array([_mp_to_l(fn(mpmath.mpf(float(u)) + mpmath.mpf(float(u - L(float(u)))))) for u in uniq], L) if len(uniq) else np.zeros(0, L)
    return out[inverse].reshape(np.shape(v))


def kvectors(kmax):
    """the half space in the order nx, then ny, then nz, ascending -> int64 [M, 3]"""
    out = [(nx, ny, nz) for nx in range(0, kmax[0] + 1) for ny in range(0 if nx == 0 else -kmax[1], kmax[1] + 1)
           for nz in range(1 if nx == 0 and ny == 0 else -kmax[2], kmax[2] + 1)]
    kv = np.array(out, np.int64).reshape(-1, 3)
    assert len(kv) == ((2 * kmax[0] + 1) * (2 * kmax[1] + 1) * (2 * kmax[2] + 1) - 1) // 2
    return kv


def set_time_constants(q, alpha, dtype):
    """tsp, a4, E_self, bgn as tgnh_set_nonbonded_ewald forms them; the sums in slot order"""
    alpha, pi, q = dtype(alpha), pi_of(dtype), q.astype(dtype)
    root = np.sqrt(pi)
    q2 = np.cumsum(q * q)[-1]
    Q = np.cumsum(q)[-1]
    return dict(tsp=(dtype(2.0) * alpha) / root, a4=dtype(4.0) * (alpha * alpha), e_self=-((dtype(K) * (alpha / root)) * q2),
                self_mag=(dtype(K) * (alpha / root)) * q2, bgn=((pi * dtype(K)) * (Q * Q)) / (dtype(2.0) * (alpha * alpha)))


def direct_terms(x, table, box, alpha, dtype, pairs=None):
    """The header's DIRECT SPACE for every ordered pair inside the cutoff (tests/test_nonbonded.py's pair_terms with the erfc lines)"""
    method, rc, eps_rf, par, ep, ex = table
    n = len(x)
    a, b = np.nonzero(~excluded_matrix(n, ep)) if pairs is None else pairs
    xs, box = x.astype(dtype), np.asarray(box, dtype)
    d = xs[a] - xs[b]
    t = d / box
    t = np.rint(t)
    t = box * t
    d = d - t
    r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    keep = r2 < dtype(rc) * dtype(rc)
    a, b, d, r2 = a[keep], b[keep], d[keep], r2[keep]
    q, sg, ep_ = (par[:, m].astype(dtype) for m in range(3))
    tsp = set_time_constants(par[:, 0], alpha, dtype)["tsp"]
    r = np.sqrt(r2)
    inv = dtype(1.0) / r
    qq = dtype(K) * (q[a] * q[b])
    sig = dtype(0.5) * (sg[a] + sg[b])
    e4 = dtype(4.0) * np.sqrt(ep_[a] * ep_[b])
    s2 = (sig * sig) / r2
    s6 = (s2 * s2) * s2
    s12 = s6 * s6
    ar = dtype(alpha) * r
    ec = _special("erfc", ar, dtype)
    g = np.exp(-(ar * ar))
    dc = qq * (-((ec * inv + tsp * g) * inv))
    dl = (e4 * (dtype(6.0) * s6 - dtype(12.0) * s12)) * inv
    c = -((dc + dl) * inv)
    return dict(a=a, b=b, d=d, c=c, r=r, r2=r2, e_c=qq * (ec * inv), e_lj=e4 * (s12 - s6),
                scale=np.abs(qq) * ((ec * inv + tsp * g) * inv) + (e4 * (dtype(6.0) * s6 + dtype(12.0) * s12)) * inv)


def exclusion_terms(x, table, alpha, dtype):
    """The header's EXCLUSION CORRECTION, for both receivers of every row with charged partners: role 0 is the row's p1"""
    par, ep = table[3], table[4]
    q = par[:, 0].astype(dtype)
    rows = np.nonzero(par[ep[:, 0], 0] * par[ep[:, 1], 0] != 0.0)[0] if len(ep) else np.zeros(0, np.int64)
    a = np.concatenate([ep[rows, 0], ep[rows, 1]]).astype(np.int64)
    b = np.concatenate([ep[rows, 1], ep[rows, 0]]).astype(np.int64)
    role = np.repeat([0, 1], len(rows))
    p1, p2 = np.concatenate([ep[rows, 0], ep[rows, 0]]).astype(np.int64), np.concatenate([ep[rows, 1], ep[rows, 1]]).astype(np.int64)
    tsp = set_time_constants(par[:, 0], alpha, dtype)["tsp"]
    xs = x.astype(dtype)
    d = xs[a] - xs[b]
    r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    qq = dtype(K) * (q[p1] * q[p2])
    zero = r2 == 0
    r = np.sqrt(np.where(zero, dtype(1.0), r2))
    inv = dtype(1.0) / r
    ar = dtype(alpha) * r
    ef = _special("erf", ar, dtype)
    g = np.exp(-(ar * ar))
    dc = qq * ((ef * inv - tsp * g) * inv)
    c = np.where(zero, dtype(0.0), -(dc * inv))
    e = np.where(zero, -(qq * tsp), -(qq * (ef * inv)))
    scale = np.where(zero, dtype(0.0), np.abs(qq) * ((ef * inv + tsp * g) * inv))
    return dict(a=a, b=b, d=d, c=c, r=r, role=role, zero=zero, e=e, scale=scale)


def reciprocal(x, q, box, alpha, kmax, dtype, chunk=256):
    """The header's RECIPROCAL SPACE -> dict force [n, 3], scale [n, 3] (the terms uncancelled), e, mag.  In float64 the sums run in
    the kernels' order; the vectors are taken `chunk` at a time to bound the memory."""
    n = len(x)
    kv = kvectors(kmax)
    pi, box = pi_of(dtype), np.asarray(box, dtype)
    a4 = set_time_constants(q, alpha, dtype)["a4"]
    q = q.astype(dtype)
    s = x.astype(dtype) / box
    s = s - np.floor(s)
    V = (box[0] * box[1]) * box[2]
    g = np.zeros((n, 3), dtype)
    scale = np.zeros((n, 3), dtype)
    terms, mags = [], []
    for m0 in range(0, len(kv), chunk):
        nv = kv[m0:m0 + chunk].astype(dtype)
        t = (s[:, 0:1] * nv[None, :, 0] + s[:, 1:2] * nv[None, :, 1]) + s[:, 2:3] * nv[None, :, 2]
        u = dtype(2.0) * (t - np.rint(t))
        sn, cs = np.sin(pi * u), np.cos(pi * u)
        Cm, Sm = np.zeros(len(nv), dtype), np.zeros(len(nv), dtype)
        Ca, Sa = np.zeros(len(nv), dtype), np.zeros(len(nv), dtype)
        for p0 in range(0, n, EW_PART):
            part = slice(p0, min(p0 + EW_PART, n))
            Cm = Cm + np.cumsum(q[part, None] * cs[part], axis=0)[-1]
            Sm = Sm + np.cumsum(q[part, None] * sn[part], axis=0)[-1]
            Ca = Ca + np.abs(q[part, None] * cs[part]).sum(0)
            Sa = Sa + np.abs(q[part, None] * sn[part]).sum(0)
        k = ((dtype(2.0) * pi) * nv) / box
        k2 = (k[:, 0] * k[:, 0] + k[:, 1] * k[:, 1]) + k[:, 2] * k[:, 2]
        A = np.exp(-(k2 / a4)) / k2
        w = (A * Cm)[None, :] * sn - (A * Sm)[None, :] * cs
        wa = (A * Ca)[None, :] * np.abs(sn) + (A * Sa)[None, :] * np.abs(cs)
        for dim in range(3):
            g[:, dim] = np.cumsum(np.concatenate([g[:, dim:dim + 1], k[None, :, dim] * w], axis=1), axis=1)[:, -1]
            scale[:, dim] += (np.abs(k[None, :, dim]) * wa).sum(1)
        terms.append(A * (Cm * Cm + Sm * Sm))
        mags.append(A * (Ca * Ca + Sa * Sa))
    pref = (dtype(8.0) * (pi * dtype(K))) / V
    pref_e = (dtype(4.0) * (pi * dtype(K))) / V
    charged = (q != 0)[:, None]
    terms = np.concatenate(terms) if terms else np.zeros(0, dtype)
    mags = np.concatenate(mags) if mags else np.zeros(0, dtype)
    return dict(force=np.where(charged, ((pref * q)[:, None]) * g, dtype(0.0)), scale=np.abs(pref * q)[:, None] * scale,
                e=pref_e * terms.sum(), mag=pref_e * mags.sum())


def evaluate(x, table, box, ewald, dtype):
    """Everything tgnh_compute_nonbonded_force adds with Ewald on -> dict: force [n, 3] (direct pairs, evaluated exceptions,
    exclusion correction, reciprocal), exact [n, 3] (the first three, as the sum of their rounded integers / 2^32: what a twin of the
    converted shares gives), recip [n, 3], scale [n, 3], count [n] conversions, energy [8], mag [8]"""
    alpha, kmax = ewald[0], tuple(int(v) for v in ewald[1:])
    n = len(x)
    pairs = searched_pairs(x, table, box)[0] if n > 1500 else None
    p = direct_terms(x, table, box, alpha, dtype, pairs)
    e = exception_terms(x, table, dtype)
    c = exclusion_terms(x, table, alpha, dtype)
    q = table[3][:, 0]
    const = set_time_constants(q, alpha, dtype)
    force, scale, count = np.zeros((n, 3), dtype), np.zeros((n, 3), dtype), np.zeros(n, np.int64)
    exact = np.zeros((n, 3), np.int64)
    for t, live in ((p, None), (e, None), (c, ~c["zero"])):
        idx = slice(None) if live is None else live
        share = t["c"][idx, None] * t["d"][idx]
        np.add.at(force, t["a"][idx], share)
        np.add.at(exact, t["a"][idx], np.rint(share.astype(np.float64) * FIXED).astype(np.int64))
        np.add.at(scale, t["a"][idx], (t["scale"][idx] / t["r"][idx])[:, None] * np.abs(t["d"][idx]))
        np.add.at(count, t["a"][idx], 1)
    M = len(kvectors(kmax))
    if M:
        r = reciprocal(x, q, box, alpha, kmax, dtype)
    else:
        r = dict(force=np.zeros((n, 3), dtype), scale=np.zeros((n, 3), dtype), e=dtype(0.0), mag=dtype(0.0))
    count = count + ((q != 0) & (M > 0))
    box = np.asarray(box, dtype)
    V = (box[0] * box[1]) * box[2]
    once, first, cfirst = p["a"] < p["b"], e["role"] == 0, c["role"] == 0
    kinds = (p["e_c"][once], p["e_lj"][once], e["e_c"][first], e["e_lj"][first])
    energy = [k.sum() for k in kinds] + [r["e"], const["e_self"], -(const["bgn"] / V), c["e"][cfirst].sum()]
    mag = [np.abs(k).sum() for k in kinds] + [r["mag"], const["self_mag"], const["bgn"] / V, np.abs(c["e"][cfirst]).sum()]
    return dict(force=force + r["force"], exact=exact, recip=r["force"], scale=scale + r["scale"], count=count,
                energy=np.array(energy, dtype), mag=np.array(mag, dtype), direct=p, exclusion=c)


# ---------------------------------------------------------------------------
# the systems and states of the GPU tests
# ---------------------------------------------------------------------------
ROCK_A, ROCK_L, ROCK_RC = 0.564, 1.128, 0.56
ROCK_EWALD = (6.0 / ROCK_RC, 24, 24, 24)
E4_SHAPE, E4_SPACING, E4_CUTOFF, E4_EWALD = (15, 14, 20), 0.4, 0.3, (3.0, 3, 4, 5)


def ions(x, q, cutoff, name):
    n = len(x)
    f = NonbondedForce()
    for i in range(n):
        f.addParticle(q[i], 0.3, 0.0)
    f.setNonbondedMethod(f.CutoffPeriodic)
    f.setCutoffDistance(cutoff)
    s = DrudeSystem(mass=np.full(n, 23.0), pair_drude=np.zeros(0, np.int32), pair_parent=np.zeros(0, np.int32), resid=np.arange(n, dtype=np.int32),
                    positions=x, velocities=np.zeros_like(x), name=name)
    return s, f.tables()


def rock_salt():
    """64 ions on a 4 x 4 x 4 lattice of spacing a / 2, charges +-1 by parity -> (system, table)"""
    if "rock" not in _cache:
        i, j, k = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
        x = np.stack([i, j, k], -1).reshape(-1, 3) * (ROCK_A / 2)
        q = np.where((i + j + k).ravel() % 2 == 0, 1.0, -1.0)
        _cache["rock"] = ions(x, q, ROCK_RC, "rock salt, 64 ions")
    return _cache["rock"]


def rock_jitter():
    return rock_salt()[0].positions + np.random.default_rng(21).normal(0, 0.01, (64, 3))


def lattice_e4():
    """4 200 ions on a jittered lattice whose spacing is above the cutoff: no pair inside it; every seventh slot has no charge"""
    if "e4" not in _cache:
        i, j, k = np.meshgrid(*(np.arange(m) for m in E4_SHAPE), indexing="ij")
        x = np.stack([i, j, k], -1).reshape(-1, 3) * E4_SPACING + np.random.default_rng(22).uniform(-0.03, 0.03, (int(np.prod(E4_SHAPE)), 3))
        q = np.where((i + j + k).ravel() % 2 == 0, 1.0, -0.75)
        q[::7] = 0.0
        _cache["e4"] = ions(x, q, E4_CUTOFF, "jittered lattice, 4200 ions")
    return _cache["e4"]


BOX_E4 = tuple(m * E4_SPACING for m in E4_SHAPE)


def ewald_b():
    """system B's parameters: alpha from a tight tolerance, kmax by the rule -- the three edges give three different ones"""
    f = NonbondedForce()
    f.setCutoffDistance(1.0)
    f.setEwaldErrorTolerance(1e-6)
    return f.ewald_parameters(BOX_B)


def ewald_a():
    f = NonbondedForce()
    f.setCutoffDistance(1.0)
    return f.ewald_parameters(BOX_A)


def charged_b():
    """system B's table with one ion's charge changed: a net charge"""
    if "charged b" not in _cache:
        s, table, info = system_b()
        par = table[3].copy()
        par[info["lonely"], 0] += 0.5
        _cache["charged b"] = table[:3] + (par,) + table[4:]
    return _cache["charged b"]


def ewald_states():
    """every (name, precision) -> (x as the device reads it, table, box, (alpha, kx, ky, kz)) the GPU tests use"""
    if "states" not in _cache:
        out = {}
        sr, tr = rock_salt()
        sa, ta = system_a()
        sb, tb, _ = system_b()
        s4, t4 = lattice_e4()
        box_r = (ROCK_L,) * 3
        for p in PRECISIONS:
            out["E1", p] = (stored(sr.positions, p)["x"], tr, box_r, ROCK_EWALD)
            out["E2", p] = (stored(sb.positions, p)["x"], tb, BOX_B, ewald_b())
            out["E2 charged", p] = (stored(sb.positions, p)["x"], charged_b(), BOX_B, ewald_b())
            out["E3", p] = (stored(sa.positions, p)["x"], ta, BOX_A, ewald_a())
        out["E1 jitter", "double"] = (stored(rock_jitter(), "double")["x"], tr, box_r, ROCK_EWALD)
        out["E2 more", "mixed"] = (stored(sb.positions, "mixed")["x"], tb, BOX_B_MORE, ewald_b())
        out["E4", "mixed"] = (stored(s4.positions, "mixed")["x"], t4, BOX_E4, E4_EWALD)
        _cache["states"] = out
    return _cache["states"]


def evaluated(name, precision, dtype):
    key = ("eval", name, precision, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = evaluate(*ewald_states()[name, precision], dtype)
    return _cache[key]


def force_gate(ref):
    """[n, 3]: what the GPU tests allow a slot's entry to be off the reference, in kJ/mol/nm"""
    return L(GATE_EWALD) * ref["scale"].astype(L) + (L(2.0) ** -33) * ref["count"][:, None].astype(L)


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def test_the_reference_gives_the_madelung_energy():
    x, table, box, ewald = ewald_states()["E1", "double"]
    r = evaluated("E1", "double", L)
    want = -L(32) * L(MADELUNG) * L(K) / L(ROCK_A / 2)
    total = r["energy"].sum()
    print(f"rock salt: {float(total):.12f} kJ/mol against {float(want):.12f}: relative {float(abs(total - want) / abs(want)):.2e}")
    assert abs(total - want) <= L(1e-14) * abs(want)
    assert np.abs(r["force"]).max() <= force_gate(r).max() and len(kvectors(ewald[1:])) == 58824


def test_the_total_does_not_depend_on_alpha_at_converged_settings():
    x, table, box, ewald = ewald_states()["E1 jitter", "double"]
    other = (6.5 / ROCK_RC, 26, 26, 26)
    for alpha, k in (ewald[:2], other[:2]):
        assert alpha * ROCK_RC >= 6 and (np.pi * k / (alpha * ROCK_L)) ** 2 >= 37
    first, second = evaluated("E1 jitter", "double", L), evaluate(x, table, box, other, L)
    off = abs(first["energy"].sum() - second["energy"].sum())
    print(f"alpha {ewald[0]:.3f} against {other[0]:.3f}: totals differ by {float(off):.2e} kJ/mol, forces by {float(np.abs(first['force'] - second['force']).max()):.2e}")
    assert off <= L(1e-14) * first["mag"].sum()
    assert np.abs(first["force"] - second["force"]).max() <= L(1e-13) * np.abs(first["force"]).max()
    assert np.abs(first["force"]).max() > 10


def small_system():
    """14 particles in a box, a net charge, four exception rows: charged partners at a distance, at r = 0, uncharged, and evaluated"""
    rng = np.random.default_rng(3)
    n = 14
    while True:
        x = rng.uniform(-1.0, 4.0, (n, 3))
        x[9] = x[8]                                              # r = 0, excluded
        f = NonbondedForce()
        for i in range(n):
            f.addParticle(rng.uniform(-1, 1) if i != 11 else 0.0, rng.uniform(0.2, 0.35), rng.uniform(0.1, 0.9))
        f.addException(0, 1, 0.3, 0.28, 0.5)
        f.addException(2, 3, 0.0, 1.0, 0.0)
        f.addException(8, 9, 0.0, 1.0, 0.0)
        f.addException(10, 11, 0.0, 1.0, 0.0)
        f.setNonbondedMethod(f.CutoffPeriodic)
        box = (2.2, 2.6, 3.1)
        t = direct_terms(x, f.tables(), box, 3.0, np.float64)
        if t["r"].min() > 0.22 and np.abs(t["r"] - 1.0).min() > 1e-3 and len(t["a"]) > 40:
            assert abs(f.tables()[3][:, 0].sum()) > 0.1
            return x, f.tables(), box


@pytest.mark.parametrize("kind", ("direct", "reciprocal", "exclusion"))
def test_forces_against_finite_differences_of_the_energy(kind):
    x, table, box = small_system()
    alpha, kmax = 3.0, (3, 4, 5)
    q = table[3][:, 0]

    def both(y):
        if kind == "direct":
            t = direct_terms(y, table[:3] + (table[3] * np.array([1.0, 1.0, 0.0]),) + table[4:], box, alpha, L)
            f = np.zeros((len(y), 3), L)
            np.add.at(f, t["a"], t["c"][:, None] * t["d"])
            return f, t["e_c"][t["a"] < t["b"]].sum()
        if kind == "reciprocal":
            r = reciprocal(y, q, box, alpha, kmax, L)
            return r["force"], r["e"]
        t = exclusion_terms(y, table, alpha, L)
        f = np.zeros((len(y), 3), L)
        np.add.at(f, t["a"], t["c"][:, None] * t["d"])
        return f, t["e"][t["role"] == 0].sum()

    force, _ = both(x.astype(L))
    if kind == "exclusion":
        t = exclusion_terms(x, table, alpha, L)
        assert t["zero"].sum() == 2 and len(t["a"]) == 6         # (10, 11) has an uncharged partner: no row
        assert not np.any(force[8]) and not np.any(force[9])
    assert np.abs(force).max() > 1.0
    h, worst = L(1e-6), L(0)
    for i in range(len(x)):
        for k in range(3):
            e = []
            for sign in (1, -1):
                y = x.astype(L)
                y[i, k] += sign * h
                e.append(both(y)[1])
            worst = max(worst, abs(-(e[0] - e[1]) / (2 * h) - force[i, k]))
    print(f"{kind}: forces off the central differences by at most {float(worst / np.abs(force).max()):.2e} of the largest")
    assert worst <= 1e-8 * np.abs(force).max()


# ---------------------------------------------------------------------------
# the states, and twin against reference
# ---------------------------------------------------------------------------
def test_the_states_have_the_shapes_the_kernels_can_go_wrong_at():
    states = ewald_states()
    seen = dict(zero=False, charged=False, outside=False, parts=False, ragged=False, three=False)
    for (name, p), (x, table, box, ewald) in states.items():
        n, rc, q = len(x), table[1], table[3][:, 0]
        if n <= 1500:
            d = x[:, None, :] - x[None, :, :]
            d -= np.asarray(box) * np.rint(d / np.asarray(box))
            r2 = (d * d).sum(-1)[~excluded_matrix(n, table[4])]
            gap = np.abs(r2 - rc ** 2).min() / rc ** 2
        else:
            pairs, gap = searched_pairs(x, table, box)
            assert len(direct_terms(x, table, box, ewald[0], np.float64, pairs)["a"]) == 0          # E4: the reciprocal part alone
        assert gap >= 1e-9, (name, p, gap)
        t, r = evaluated(name, p, np.float64), evaluated(name, p, L)
        assert np.array_equal(t["direct"]["a"], r["direct"]["a"]) and np.array_equal(t["direct"]["b"], r["direct"]["b"])
        M = len(kvectors(ewald[1:]))
        seen["zero"] |= bool(r["exclusion"]["zero"].any())
        seen["charged"] |= abs(q.sum()) > 0.1
        seen["outside"] |= bool((x > np.asarray(box)).any() and (x < 0).any())
        seen["parts"] |= n > EW_PART and n % EW_PART != 0
        seen["ragged"] |= M % 64 != 0
        seen["three"] |= len(set(ewald[1:])) == 3 and len(set(box)) == 3
        assert np.array_equal(stored(x, p)["x"], x)              # the state is what the precision stores
    assert all(seen.values()), seen
    assert len(kvectors(E4_EWALD[1:])) == 346 and len(lattice_e4()[0].positions) == 4200
    x3 = ewald_states()["E3", "double"][0]
    assert np.array_equal(x3[0::5], x3[1::5])                    # system A: every Drude particle exactly on its oxygen


def margins():
    if "margins" not in _cache:
        out = {"force": 0.0, **{k: 0.0 for k in ENERGIES}}
        for (name, p) in ewald_states():
            t, r = evaluated(name, p, np.float64), evaluated(name, p, L)
            live = r["scale"] > 0
            if live.any():
                out["force"] = max(out["force"], float((np.abs(t["force"].astype(L) - r["force"])[live] / r["scale"][live]).max()))
            assert not np.any(t["force"][~live]) and not np.any(r["force"][~live])
            for m, kind in enumerate(ENERGIES):
                if r["mag"][m] > 0:
                    out[kind] = max(out[kind], float(abs(L(t["energy"][m]) - r["energy"][m]) / r["mag"][m]))
                else:
                    assert t["energy"][m] == 0 and r["energy"][m] == 0
        _cache["margins"] = out
    return _cache["margins"]


def test_the_margins_between_twin_and_reference():
    m = margins()
    for kind, v in m.items():
        print(f"twin against reference, {kind}: {v:.3e}")
    worst = max(m.values())
    print(f"the largest: {worst:.3e}; MEASURED_MARGIN_EWALD {MEASURED_MARGIN_EWALD:.1e}, GATE_EWALD {GATE_EWALD:.1e}")
    assert MEASURED_MARGIN_EWALD / 4 < worst <= MEASURED_MARGIN_EWALD


def test_the_twins_direct_and_exclusion_shares_cancel_exactly():
    for name in ("E2 charged", "E3"):
        t = evaluated(name, "mixed", np.float64)
        assert np.array_equal(t["exact"].sum(0), np.zeros(3, np.int64)) and np.any(t["exact"] != 0)


# ---------------------------------------------------------------------------
# ewald_parameters
# ---------------------------------------------------------------------------
def test_the_parameter_rule_on_a_water_box():
    s, table = system_a()
    x = np.asarray(s.positions, np.float64)
    f = NonbondedForce()
    f.setCutoffDistance(1.0)
    assert f.getEwaldErrorTolerance() == 5e-4 and f.getEwaldParameters() == (0.0, 0, 0, 0)
    alpha, kx, ky, kz = f.ewald_parameters(BOX_A)
    assert alpha == math.sqrt(-math.log(2.0 * 5e-4)) and kx == ky == kz >= 1
    assert f.ewald_parameters(np.diag(BOX_A)) == (alpha, kx, ky, kz)
    err = lambda k: k * np.sqrt(BOX_A[0] * alpha) / 20 * np.exp(-(np.pi * k / (BOX_A[0] * alpha)) ** 2)      # noqa: E731
    assert err(kx) <= 5e-4 and (kx == 1 or err(kx - 1) > 5e-4)
    # the converged force: a wider cutoff than the table's is not to be had (half the box), so alpha rc = 4 (erfc(4) = 1.5e-8) with kmax 24 ((pi kmax / (alpha L))^2 = 20)
    converged = evaluate(x, table, BOX_A, (4.0, 24, 24, 24), np.float64)["force"]
    errors = []
    for tol in (5e-4, 1e-5):
        f.setEwaldErrorTolerance(tol)
        got = evaluate(x, table, BOX_A, f.ewald_parameters(BOX_A), np.float64)["force"]
        errors.append(float(np.sqrt(((got - converged) ** 2).sum(1).mean())))
        print(f"tolerance {tol:.0e}: parameters {f.ewald_parameters(BOX_A)}, RMS force error {errors[-1]:.3e} kJ/mol/nm, "
              f"{errors[-1] / np.sqrt((converged ** 2).sum(1).mean()):.2e} of the RMS force: error / tolerance {errors[-1] / tol:.2f}")
    assert errors[1] < errors[0] / 10
    f.setEwaldParameters(2.5, 3, 4, 5)
    assert f.getEwaldParameters() == (2.5, 3, 4, 5) == f.ewald_parameters(BOX_A)


# ---------------------------------------------------------------------------
# tgnh_set_nonbonded_ewald on a host-only handle; the table class; NonbondedForces
# ---------------------------------------------------------------------------
def desc(alpha=3.0, kmax=(3, 4, 5), size=None):
    return _lib.TgnhEwaldDesc(C.sizeof(_lib.TgnhEwaldDesc) if size is None else size, (C.c_int32 * 3)(*kmax), alpha)


def test_refusals_on_a_host_only_handle():
    s, table, info = system_b()
    top = HostTopology(s, integrator())
    lib = top.lib
    assert C.sizeof(_lib.TgnhEwaldDesc) == 24
    assert lib.tgnh_set_nonbonded_ewald(None, None) == _lib.ERR_ARG
    assert lib.tgnh_set_nonbonded_ewald(top.h, C.byref(desc())) == _lib.ERR_STATE and "no nonbonded table" in lib.tgnh_last_error().decode()
    assert lib.tgnh_set_nonbonded_ewald(top.h, None) == _lib.TGNH_OK              # nothing to clear: fine
    f = NonbondedForces(top, table)
    assert f.ewald is None
    f.set_ewald(2.5, 1, 2, 3)
    assert f.ewald == (2.5, (1, 2, 3), (3 * 5 * 7 - 1) // 2)
    bad = [(desc(size=16), _lib.ERR_ARG, "struct_size 16"), (desc(alpha=0.0), _lib.ERR_ARG, "alpha is not finite or not positive"),
           (desc(alpha=-1.0), _lib.ERR_ARG, "alpha is not finite"), (desc(alpha=np.nan), _lib.ERR_ARG, "alpha is not finite"),
           (desc(alpha=np.inf), _lib.ERR_ARG, "alpha is not finite"), (desc(kmax=(3, -1, 5)), _lib.ERR_ARG, r"kmax[1] = -1"),
           (desc(kmax=(3, 4, 256)), _lib.ERR_ARG, "kmax[2] = 256"), (desc(kmax=(64, 64, 64)), _lib.ERR_UNSUPPORTED, "more than 2^20")]
    for d, status, text in bad:
        assert lib.tgnh_set_nonbonded_ewald(top.h, C.byref(d)) == status, text
        assert text in lib.tgnh_last_error().decode()
        assert f.ewald == (2.5, (1, 2, 3), 52)                   # a refused call leaves what was in force
    assert lib.tgnh_set_nonbonded_ewald(top.h, C.byref(desc(kmax=(63, 63, 64)))) == _lib.TGNH_OK     # M = 1 040 320 <= 2^20
    assert f.ewald[2] == (127 * 127 * 129 - 1) // 2 <= 2 ** 20
    f.set_ewald(2.5, 0, 0, 0)
    assert f.ewald == (2.5, (0, 0, 0), 0)                        # legal: no reciprocal part
    assert lib.tgnh_get_nonbonded_ewald(top.h, None, None) == _lib.ERR_ARG
    e = _lib.TgnhEwaldDesc()
    assert lib.tgnh_get_nonbonded_ewald(top.h, C.byref(e), None) == _lib.TGNH_OK and e.struct_size == 24
    for call in (f.ewald_energy,):
        with pytest.raises(TgnhError, match="host-only") as err:
            call()
        assert err.value.status == _lib.ERR_STATE
    assert lib.tgnh_get_ewald_energy(top.h, None, None) == _lib.ERR_ARG
    # tgnh_set_nonbonded_force drops the setting: a new table, and a clearing call
    f.set_ewald(2.5, 1, 2, 3)
    f = NonbondedForces(top, table)
    assert f.ewald is None
    f.set_ewald(2.5, 1, 2, 3)
    f.clear_ewald()
    assert f.ewald is None
    f.set_ewald(2.5, 1, 2, 3)
    f.clear()
    assert f.ewald is None and f.num_terms == (0, 0, 0)
    top.close()


def test_the_table_class():
    f = NonbondedForce()
    assert f.Ewald == 3 and (f.NoCutoff, f.CutoffNonPeriodic, f.CutoffPeriodic) == (0, 1, 2)
    f.setNonbondedMethod(f.Ewald)
    assert f.getNonbondedMethod() == 3
    with pytest.raises(ValueError):
        f.setNonbondedMethod(7)
    with pytest.raises(ValueError):
        f.setNonbondedMethod(4)
    assert f.getEwaldErrorTolerance() == 5e-4
    f.setEwaldErrorTolerance(1e-5)
    assert f.getEwaldErrorTolerance() == 1e-5
    f.setEwaldParameters(3.5, 7, 8, 9)
    assert f.getEwaldParameters() == (3.5, 7, 8, 9)
    f.setEwaldParameters(0, 0, 0, 0)
    a = f.ewald_parameters((2.0, 3.0, 4.0))
    assert a[0] == math.sqrt(-math.log(2.0 * 1e-5)) and a[1] < a[2] < a[3]
    f.addParticle(1.0, 0.3, 0.1)
    assert len(f.tables()) == 6 and f.tables()[0] == 3


def test_the_three_ways_in():
    s, table, info = system_b()
    top = HostTopology(s, integrator())
    f = NonbondedForce()
    for row in table[3]:
        f.addParticle(*row)
    for (p1, p2), row in zip(table[4], table[5]):
        f.addException(int(p1), int(p2), *row)
    f.setCutoffDistance(1.0)
    f.setNonbondedMethod(f.Ewald)
    # an Ewald-method object on an owner without a box: refused before any library call
    with pytest.raises(TgnhError, match="setPeriodicBoxVectors first, or pass ewald=") as e:
        NonbondedForces(top, f)
    assert e.value.status == _lib.ERR_STATE
    out = (C.c_int * 3)()
    assert top.lib.tgnh_get_num_nonbonded_terms(top.h, out) == 0 and tuple(out) == (0, 0, 0)
    nb = NonbondedForces(top, f, ewald=(2.5, 1, 2, 3))           # ... unless the parameters come along
    assert nb.ewald == (2.5, (1, 2, 3), 52) and nb.num_terms[0] == s.num_particles
    top.setPeriodicBoxVectors((BOX_B[0], 0, 0), (0, BOX_B[1], 0), (0, 0, BOX_B[2]))
    nb = NonbondedForces(top, f)                                 # from the owner's box and the tolerance
    want = f.ewald_parameters(BOX_B)
    assert nb.ewald[0] == want[0] and nb.ewald[1] == tuple(want[1:]) and len(set(want[1:])) == 3
    f.setEwaldParameters(3.0, 2, 2, 2)
    assert NonbondedForces(top, f).ewald == (3.0, (2, 2, 2), 62)
    # a method-2 tuple with ewald=
    nb = NonbondedForces(top, table, ewald=(2.0, 1, 1, 1))
    assert nb.ewald == (2.0, (1, 1, 1), 13)
    assert NonbondedForces(top, table).ewald is None
    with pytest.raises(TgnhError, match="ewald: ") as e:
        NonbondedForces(top, table, ewald=(2.0, 1, 1))
    assert e.value.status == _lib.ERR_ARG
    # a raw tuple with method 3 is refused exactly as before
    with pytest.raises(TgnhError, match="only TGNH_NB_CUTOFF_PERIODIC") as e:
        NonbondedForces(top, (3,) + table[1:])
    assert e.value.status == _lib.ERR_UNSUPPORTED
    with pytest.raises(TgnhError, match="only TGNH_NB_CUTOFF_PERIODIC"):
        NonbondedForces(top, (3,) + table[1:], ewald=(2.0, 1, 1, 1))
    top.close()
