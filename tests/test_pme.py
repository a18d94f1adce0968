"""Smooth particle-mesh Ewald on the library's NonbondedForce without a GPU (csrc/tgnh_pme.*; include/drude_tgnh.h, PARTICLE-MESH
EWALD, has the contract): an fp80 REFERENCE, an fp64 numpy TWIN, the states the GPU tests run (tests/test_pme_gpu.py), and the checks
that need no device.  Everything PME shares with the explicit sum (erfc pairs, exclusion correction, self and background energies)
comes from tests/test_ewald.py's reference, asked for kmax (0, 0, 0).

 * THE REFERENCE restates the header in np.longdouble; its DFT is done by per-axis matrices W[j, k] = exp(-2 pi i ((j k) mod N) / N),
   so it rests on no FFT library.  It is held to: agreement with tests/test_ewald.py's fp80 explicit sum at one alpha with kmax
   converged, the RMS force deviation falling by at least 8 at each of two doublings of the grid (order 5 predicts 32 asymptotically;
   the figures are printed); central differences of its own reciprocal energy within 1e-8 of the largest force; the sum of the
   reciprocal forces falling with the grid (printed, not gated: PME does not conserve momentum exactly).
 * THE TWIN is the same code on float64 with np.fft.  Its integer charge grid follows the header operation for operation and is
   what the GPU tests ask the device for bit for bit (B-splines need no math library); behind the grid np.fft's order of operations
   is not the device's, so phi, forces and energy are not.
 * MEASURED_MARGIN_PME.  The twin's largest deviation from the reference over every state of the GPU tests, relative to uncancelled
   terms: a slot's reciprocal force component relative to K |q| (N_d / L_d) sum_abc |dth th th| Phi_abs, Phi_abs the absolute value of
   the real-space kernel convolved with |Q|; the reciprocal energy relative to 1/2 K (sum |Q|)^2 sum G; phi on the transform-only
   grids relative to Phi_abs; the whole call's force relative to that plus tests/test_ewald.py's S_i; the other seven energies
   relative to that file's magnitudes.  test_the_margins prints every figure; the constant is the largest.  GATE_PME = 16 x that,
   the project's factor.
 * CONDITIONS on the states, asserted here: a support that wraps the boundary in every axis; a slot with s = 0 exactly; slots at
   negative coordinates and two box lengths outside; an excluded pair at r = 0; a net charge; a slot with q = 0; grids with all three
   radices in one line; a pure-radix line each (16, 27, 25); three thin grids that reach the longest lines; the modulus rule
   exercised on every even N, and no modulus below 1e-7 afterwards.
 * every refusal of tgnh_set_nonbonded_pme on a host-only handle with its status and text, nothing changed afterwards; the one
   setting with two forms; pme_parameters; NonbondedForces' ways in."""
import ctypes as C
import math

import numpy as np
import pytest

from openmm_drudenose_amd import _lib
from openmm_drudenose_amd.drudetgnhplugin import HostTopology, TgnhError
from openmm_drudenose_amd.forces import NonbondedForce, NonbondedForces
from test_nonbonded import PRECISIONS, K, L, BOX_A, BOX_B, BOX_B_MORE, system_a, system_b, stored, integrator
from test_ewald import (ENERGIES, MADELUNG, ROCK_A, ROCK_L, ROCK_EWALD, BOX_E4, evaluate, reciprocal, pi_of, rock_salt, rock_jitter, lattice_e4,
                        charged_b, ewald_b, small_system)

# test_the_margins_between_twin_and_reference prints the figures; when this was written the largest was the whole call's force, 8.0e-14
# (its direct part, as in tests/test_ewald.py: the pair Lennard-Jones energy gave 6.4e-14); the mesh's own figures are far below it:
# reciprocal force 8.6e-16, phi 2.8e-16, reciprocal energy 2.1e-17
MEASURED_MARGIN_PME = 8.5e-14
GATE_PME = 16 * MEASURED_MARGIN_PME
ORDER = 5
PME_FIXED = 2.0 ** 48
THIN_GRIDS = ((256, 6, 6), (6, 250, 6), (6, 6, 243))
MIXED_GRIDS = ((10, 12, 15), (20, 24, 30))
GRID_P1, GRID_P2, GRID_P4 = (32, 30, 36), (20, 24, 30), (16, 27, 25)
_cache = {}


# ---------------------------------------------------------------------------
# the terms of the header
# ---------------------------------------------------------------------------
def weights(x, edge, N, dtype):
    """WEIGHTS for one axis -> i0 [n] int64, th [5, n], dth [5, n]"""
    x, edge = np.asarray(x, dtype), dtype(edge)
    s = x / edge
    s = s - np.floor(s)
    t = s * dtype(N)
    fl = np.floor(t)
    u = t - fl
    th = np.zeros((ORDER, len(x)), dtype)
    th[0], th[1] = dtype(1.0) - u, u

    def raise_to(k):
        div = dtype(k - 1)
        th[k - 1] = (u * th[k - 2]) / div
        for j in range(1, k - 1):
            th[k - 1 - j] = ((u + dtype(j)) * th[k - 2 - j] + (dtype(k - j) - u) * th[k - 1 - j]) / div
        th[0] = ((dtype(1.0) - u) * th[0]) / div

    raise_to(3)
    raise_to(4)
    dth = np.zeros_like(th)
    dth[0] = -th[0]
    for j in range(1, ORDER):
        dth[j] = th[j - 1] - th[j]
    raise_to(5)
    return fl.astype(np.int64), th, dth


def all_weights(x, box, grid, dtype):
    return [weights(x[:, d], box[d], grid[d], dtype) for d in range(3)]


def spread(q, w, grid, dtype):
    """SPREADING -> Q int64 [nz, ny, nx]"""
    nx, ny, nz = grid
    (ix, thx, _), (iy, thy, _), (iz, thz, _) = w
    live = np.nonzero(q != 0)[0]
    qq = q.astype(dtype)[live]
    Q = np.zeros((nz, ny, nx), np.int64)
    for c in range(ORDER):
        for b in range(ORDER):
            for a in range(ORDER):
                wgt = (thx[a, live] * thy[b, live]) * thz[c, live]
                v = np.rint((qq * wgt) * dtype(PME_FIXED)).astype(np.int64)
                np.add.at(Q, ((iz[live] + c) % nz, (iy[live] + b) % ny, (ix[live] + a) % nx), v)
    return Q


def moduli(N, dtype):
    """|b(m)|^2 with OpenMM's rule -> (table [N], the m the rule replaced)"""
    M = [dtype(1.0) / dtype(24.0), dtype(11.0) / dtype(24.0), dtype(11.0) / dtype(24.0), dtype(1.0) / dtype(24.0)]
    m = np.arange(N)
    sc, ss = np.zeros(N, dtype), np.zeros(N, dtype)
    for j in range(4):
        ang = (dtype(2.0) * pi_of(dtype)) * ((m * j) % N).astype(dtype) / dtype(N)
        sc = sc + M[j] * np.cos(ang)
        ss = ss + M[j] * np.sin(ang)
    b = sc * sc + ss * ss
    replaced = []
    for k in range(N):
        if b[k] < 1e-7:
            b[k] = (b[(k - 1 + N) % N] + b[(k + 1) % N]) * dtype(0.5)
            replaced.append(k)
    return b, replaced


def influence(box, alpha, grid, dtype):
    """INFLUENCE FUNCTION -> G [nz, ny, nx]"""
    pi, box = pi_of(dtype), np.asarray(box, dtype)
    pi2, alpha2 = pi * pi, dtype(alpha) * dtype(alpha)
    h, b = [], []
    for d in range(3):
        m = np.arange(grid[d])
        n = np.where(m <= grid[d] // 2, m, m - grid[d]).astype(dtype)
        h.append(n / box[d])
        b.append(moduli(grid[d], dtype)[0])
    hx, hy, hz = h[0][None, None, :], h[1][None, :, None], h[2][:, None, None]
    bx, by, bz = b[0][None, None, :], b[1][None, :, None], b[2][:, None, None]
    m2 = (hx * hx + hy * hy) + hz * hz
    m2[0, 0, 0] = dtype(1.0)
    V = (box[0] * box[1]) * box[2]
    G = np.exp(-((pi2 * m2) / alpha2)) / (((pi * V) * m2) * ((bx * by) * bz))
    G[0, 0, 0] = dtype(0.0)
    return G


def dft3(A, inverse, dtype):
    """the unnormalised 3-D DFT of A [nz, ny, nx]; in longdouble by per-axis matrices, in float64 by np.fft"""
    if dtype is not L:
        return np.fft.ifftn(A) * A.size if inverse else np.fft.fftn(A)
    A = A.astype(np.clongdouble)
    for axis in range(3):
        N = A.shape[axis]
        j = np.arange(N)
        ang = (L(2.0) * pi_of(L)) * ((j[:, None] * j[None, :]) % N).astype(L) / L(N)
        W = np.cos(ang) + (1j if inverse else -1j) * np.sin(ang)
        A = np.moveaxis(np.tensordot(W, A, axes=([1], [axis])), 0, axis)
    return A


def potential(Q, box, alpha, dtype):
    """TRANSFORMS -> phi [nz, ny, nx], F, G from the integer grid"""
    grid = Q.shape[::-1]
    G = influence(box, alpha, grid, dtype)
    F = dft3(Q.astype(dtype) * dtype(1.0 / PME_FIXED), False, dtype)
    phi = dft3(G * F, True, dtype).real
    return phi, F, G


def phi_abs(Q, G):
    """|the real-space kernel| convolved with |Q| 2^-48, in float64 (a scale, not a reference)"""
    G = G.astype(np.float64)
    kern = np.abs((np.fft.ifftn(G) * G.size).real)
    return np.fft.ifftn(np.fft.fftn(kern) * np.fft.fftn(np.abs(Q).astype(np.float64) / PME_FIXED)).real


def pme_reciprocal(x, q, box, alpha, grid, dtype):
    """The header's mesh sum -> dict Q, phi, force [n, 3], scale [n, 3] (the terms uncancelled), e, mag, phi_abs"""
    n = len(x)
    nx, ny, nz = grid
    w = all_weights(x, box, grid, dtype)
    Q = spread(q, w, grid, dtype)
    phi, F, G = potential(Q, box, alpha, dtype)
    pa = phi_abs(Q, G)
    (ix, thx, dthx), (iy, thy, dthy), (iz, thz, dthz) = w
    g, sc = np.zeros((3, n), dtype), np.zeros((3, n), np.float64)
    for c in range(ORDER):
        for b in range(ORDER):
            for a in range(ORDER):
                at = ((iz + c) % nz, (iy + b) % ny, (ix + a) % nx)
                p, ap = phi[at], pa[at]
                terms = ((dthx[a] * thy[b]) * thz[c], (thx[a] * dthy[b]) * thz[c], (thx[a] * thy[b]) * dthz[c])
                for d in range(3):
                    g[d] = g[d] + terms[d] * p
                    sc[d] += np.abs(terms[d].astype(np.float64)) * ap
    qd, boxd = q.astype(dtype), np.asarray(box, dtype)
    force, scale = np.zeros((n, 3), dtype), np.zeros((n, 3), np.float64)
    for d in range(3):
        force[:, d] = -(((dtype(K) * qd) * (dtype(grid[d]) / boxd[d])) * g[d])
        scale[:, d] = K * np.abs(q) * (grid[d] / box[d]) * sc[d]
    charged = (q != 0)[:, None]
    absq = np.abs(Q).astype(dtype).sum() * dtype(1.0 / PME_FIXED)
    return dict(Q=Q, phi=phi, phi_abs=pa, force=np.where(charged, force, dtype(0.0)), scale=np.where(charged, scale, 0.0),
                e=(dtype(0.5) * dtype(K)) * (G * (F.real * F.real + F.imag * F.imag)).sum(), mag=(dtype(0.5) * dtype(K)) * (absq * absq) * G.sum())


def pme_evaluate(x, table, box, pme, dtype):
    """Everything tgnh_compute_nonbonded_force adds with PME on -> tests/test_ewald.py's dict, the reciprocal part being the mesh's;
    also Q and phi"""
    alpha, grid = pme[0], tuple(int(v) for v in pme[1:])
    rest = evaluate(x, table, box, (alpha, 0, 0, 0), dtype)
    q = table[3][:, 0]
    r = pme_reciprocal(x, q, box, alpha, grid, dtype)
    energy, mag = rest["energy"].copy(), rest["mag"].copy()
    energy[4], mag[4] = r["e"], r["mag"]
    return dict(force=rest["force"] + r["force"], recip=r["force"], scale=rest["scale"] + r["scale"].astype(dtype), recip_scale=r["scale"],
                count=rest["count"] + (q != 0), energy=energy, mag=mag, Q=r["Q"], phi=r["phi"], phi_abs=r["phi_abs"], exclusion=rest["exclusion"])


# ---------------------------------------------------------------------------
# the states of the GPU tests
# ---------------------------------------------------------------------------
def pme_a():
    """the water box at the default tolerance's parameters"""
    f = NonbondedForce()
    f.setCutoffDistance(1.0)
    return f.pme_parameters(BOX_A)


def pme_states():
    """every (name, precision) -> (x as the device reads it, table, box, (alpha, nx, ny, nz)) the GPU tests compare forces and energies on"""
    if "states" not in _cache:
        out = {}
        sr, tr = rock_salt()
        sa, ta = system_a()
        sb, tb, _ = system_b()
        s4, t4 = lattice_e4()
        box_r = (ROCK_L,) * 3
        alpha_b = ewald_b()[0]
        for p in PRECISIONS:
            out["P1", p] = (stored(sr.positions, p)["x"], tr, box_r, (ROCK_EWALD[0],) + GRID_P1)
            out["P2", p] = (stored(sb.positions, p)["x"], charged_b(), BOX_B, (alpha_b,) + GRID_P2)
            out["P3", p] = (stored(sa.positions, p)["x"], ta, BOX_A, pme_a())
        out["P2 more", "mixed"] = (stored(sb.positions, "mixed")["x"], charged_b(), BOX_B_MORE, (alpha_b,) + GRID_P2)
        out["P4", "mixed"] = (stored(s4.positions, "mixed")["x"], t4, BOX_E4, (3.0,) + GRID_P4)
        _cache["states"] = out
    return _cache["states"]


def pme_evaluated(name, precision, dtype):
    key = ("eval", name, precision, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = pme_evaluate(*pme_states()[name, precision], dtype)
    return _cache[key]


def phi_state():
    """the transform-only checks: the jittered rock salt, its box stretched to three different edges"""
    sr, tr = rock_salt()
    return stored(rock_jitter(), "double")["x"], tr, (ROCK_L, 1.25 * ROCK_L, 1.5 * ROCK_L), 6.0


def phi_checked(grid, dtype):
    """-> (Q of the twin, phi in dtype from that Q, Phi_abs) on phi_state at `grid`"""
    key = ("phi", grid, np.dtype(dtype).name)
    if key not in _cache:
        x, table, box, alpha = phi_state()
        Q = spread(table[3][:, 0], all_weights(x, box, grid, np.float64), grid, np.float64)
        phi, F, G = potential(Q, box, alpha, dtype)
        _cache[key] = (Q, phi, phi_abs(Q, G))
    return _cache[key]


def force_gate(ref):
    """[n, 3]: what the GPU tests allow a slot's entry to be off the reference, in kJ/mol/nm"""
    return L(GATE_PME) * ref["scale"].astype(L) + (L(2.0) ** -33) * ref["count"][:, None].astype(L)


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
def random_charges():
    rng = np.random.default_rng(11)
    x = rng.uniform(0, 1, (300, 3)) * np.array([2.0, 2.3, 2.6])
    q = rng.uniform(-1, 1, 300)
    assert abs(q.sum()) > 1.0
    return x, q, (2.0, 2.3, 2.6), 3.0


def test_the_reference_converges_to_the_explicit_sum():
    x, q, box, alpha = random_charges()
    kmax = (14, 16, 18)
    assert all((np.pi * k / (alpha * e)) ** 2 > 50 for k, e in zip(kmax, box))          # exp(-50) = 2e-22: converged
    want = reciprocal(x, q, box, alpha, kmax, L)
    rms = np.sqrt((want["force"] ** 2).sum(1).mean())
    errors = []
    for grid in ((10, 12, 15), (20, 24, 30), (40, 48, 60)):
        got = pme_reciprocal(x, q, box, alpha, grid, L)
        errors.append(float(np.sqrt(((got["force"] - want["force"]) ** 2).sum(1).mean()) / rms))
        print(f"grid {grid}: RMS force deviation {errors[-1]:.3e} of the RMS force, energy off by {float(abs(got['e'] - want['e']) / abs(want['e'])):.3e}, "
              f"sum of the forces {np.abs(got['force'].sum(0)).max() / float(rms):.3e} of the RMS force")
    print(f"ratios at the two doublings: {errors[0] / errors[1]:.1f}, {errors[1] / errors[2]:.1f}")
    assert errors[0] / errors[1] >= 8 and errors[1] / errors[2] >= 8


def test_forces_against_finite_differences_of_the_reciprocal_energy():
    x, table, box = small_system()
    q, alpha, grid = table[3][:, 0], 3.0, (20, 24, 30)
    force = pme_reciprocal(x, q, box, alpha, grid, L)["force"]
    assert np.abs(force).max() > 1.0
    # (the charge grid is quantised at 2^-48: the differences carry that noise divided by 2 h, 2e-8 of the largest force at h = 1e-6 and
    # 2e-7 at 1e-7, while the truncation grows as h^2, 3e-8 at 1e-4: h = 1e-5 sits between the two)
    h, worst = 1e-5, L(0)
    for i in range(len(x)):
        for k in range(3):
            e = []
            for sign in (1, -1):
                y = x.astype(L)
                y[i, k] += sign * L(h)
                w = all_weights(y, box, grid, L)
                Q = spread(q, w, grid, L)
                _, F, G = potential(Q, box, alpha, L)
                e.append((L(0.5) * L(K)) * (G * (F.real * F.real + F.imag * F.imag)).sum())
            worst = max(worst, abs(-(e[0] - e[1]) / (2 * L(h)) - force[i, k]))
    print(f"reciprocal: forces off the central differences by at most {float(worst / np.abs(force).max()):.2e} of the largest")
    assert worst <= 1e-8 * np.abs(force).max()


def test_the_rock_salt_total_tends_to_the_madelung_energy():
    """a record: the mesh's error at three grids, not a gate"""
    x, table, box, pme = pme_states()["P1", "double"]
    want = -L(32) * L(MADELUNG) * L(K) / L(ROCK_A / 2)
    rest = evaluate(x, table, box, (pme[0], 0, 0, 0), L)["energy"]
    off = []
    for n in (16, 32, 64):
        r = pme_reciprocal(x, table[3][:, 0], box, pme[0], (n, n, n), L)
        off.append(float(abs(rest.sum() + r["e"] - want) / abs(want)))
        print(f"rock salt, grid {n}^3: total off the Madelung energy by {off[-1]:.3e} of it")
    assert off[2] < off[1] < off[0]


# ---------------------------------------------------------------------------
# the states, and twin against reference
# ---------------------------------------------------------------------------
def test_the_states_have_the_shapes_the_kernels_can_go_wrong_at():
    seen = dict(wraps=False, zero_s=False, outside=False, r0=False, charged=False, q0=False)
    for (name, p), (x, table, box, pme) in pme_states().items():
        grid, q = pme[1:], table[3][:, 0]
        w = all_weights(x, box, grid, np.float64)
        seen["wraps"] |= all(bool((w[d][0][q != 0] + ORDER - 1 >= grid[d]).any()) for d in range(3))
        seen["zero_s"] |= bool(((x / np.asarray(box) - np.floor(x / np.asarray(box))) == 0).any())
        seen["outside"] |= bool((x > 2 * np.asarray(box)).any() and (x < 0).any())
        seen["charged"] |= abs(q.sum()) > 0.1
        seen["q0"] |= bool((q == 0).any())
        seen["r0"] |= bool(pme_evaluated(name, p, np.float64)["exclusion"]["zero"].any())
        for d in range(3):
            assert NonbondedForce._smooth(grid[d]) and 6 <= grid[d] <= 256
            assert np.all(w[d][0] >= 0) and np.all(w[d][0] <= grid[d])
            assert np.all(np.abs(w[d][1].sum(0) - 1) < 1e-14) and np.all(np.abs(w[d][2].sum(0)) < 1e-14)      # a partition of unity
    assert all(seen.values()), seen
    radices = lambda n: {r for r in (2, 3, 5) if n % r == 0}                                                   # noqa: E731
    assert all(radices(n) == {2, 3, 5} for n in (30,)) and GRID_P2[2] == 30 and MIXED_GRIDS[1][2] == 30
    assert [radices(n) for n in GRID_P4] == [{2}, {3}, {5}]
    assert [g[d] for d, g in enumerate(THIN_GRIDS)] == [256, 250, 243] and all(np.prod(g) < 10000 for g in THIN_GRIDS)
    for grid in THIN_GRIDS + MIXED_GRIDS + (GRID_P1, GRID_P2, GRID_P4, pme_a()[1:]):
        for n in grid:
            for dtype in (np.float64, L):
                b, replaced = moduli(n, dtype)
                assert replaced == ([n // 2] if n % 2 == 0 else []) and np.all(b >= 1e-7)


def margins():
    if "margins" not in _cache:
        out = {"force": 0.0, "reciprocal force": 0.0, "phi": 0.0, **{k: 0.0 for k in ENERGIES}}
        for (name, p) in pme_states():
            t, r = pme_evaluated(name, p, np.float64), pme_evaluated(name, p, L)
            for kind, a, b, s in (("force", t["force"], r["force"], r["scale"]), ("reciprocal force", t["recip"], r["recip"], r["recip_scale"])):
                live = s > 0
                out[kind] = max(out[kind], float((np.abs(a.astype(L) - b)[live] / s[live]).max()))
                assert not np.any(a[~live]) and not np.any(b[~live])
            for m, kind in enumerate(ENERGIES):
                if r["mag"][m] > 0:
                    out[kind] = max(out[kind], float(abs(L(t["energy"][m]) - r["energy"][m]) / r["mag"][m]))
                else:
                    assert t["energy"][m] == 0 and r["energy"][m] == 0
        for grid in THIN_GRIDS + MIXED_GRIDS:
            (_, a, s), (_, b, _) = phi_checked(grid, np.float64), phi_checked(grid, L)
            out["phi"] = max(out["phi"], float((np.abs(a.astype(L) - b) / s).max()))
        _cache["margins"] = out
    return _cache["margins"]


def test_the_margins_between_twin_and_reference():
    m = margins()
    for kind, v in m.items():
        print(f"twin against reference, {kind}: {v:.3e}")
    worst = max(m.values())
    print(f"the largest: {worst:.3e}; MEASURED_MARGIN_PME {MEASURED_MARGIN_PME:.1e}, GATE_PME {GATE_PME:.1e}")
    assert MEASURED_MARGIN_PME / 4 < worst <= MEASURED_MARGIN_PME


def test_the_twins_charge_grid_sums_to_the_net_charge():
    """sum of the weights is 1: the grid's sum is the net charge to the rounding of 125 n contributions"""
    for name in ("P2", "P4"):
        x, table, box, pme = pme_states()[name, "mixed"]
        Q = pme_evaluated(name, "mixed", np.float64)["Q"]
        q = table[3][:, 0]
        assert abs(int(Q.sum()) - q.sum() * PME_FIXED) <= 125 * len(q) and np.abs(Q).max() < 2 ** 62


# ---------------------------------------------------------------------------
# pme_parameters
# ---------------------------------------------------------------------------
def test_the_parameter_rule():
    f = NonbondedForce()
    f.setCutoffDistance(1.0)
    assert f.getPMEParameters() == (0.0, 0, 0, 0)
    alpha, nx, ny, nz = f.pme_parameters((4.2, 4.2, 4.2))
    assert alpha == math.sqrt(-math.log(2.0 * 5e-4)) and abs(alpha - 2.63) < 0.005 and nx == ny == nz == 36
    assert f.pme_parameters(np.diag((4.2, 4.2, 4.2))) == (alpha, 36, 36, 36)
    assert math.ceil(2 * alpha * 4.2 / (3 * 5e-4 ** 0.2)) == 34                      # 34 = 2 17 and 35 = 5 7 are passed over
    assert f.pme_parameters((0.3, 2.0, 4.2))[1:] == (6, 18, 36)                      # at least 6
    f.setEwaldErrorTolerance(1e-5)
    fine = f.pme_parameters((4.2, 4.2, 4.2))
    assert fine[0] > alpha and fine[1] > 36 and NonbondedForce._smooth(fine[1])
    f.setPMEParameters(3.0, 20, 24, 30)
    assert f.getPMEParameters() == (3.0, 20, 24, 30) == f.pme_parameters(BOX_A)


# ---------------------------------------------------------------------------
# tgnh_set_nonbonded_pme on a host-only handle; NonbondedForces
# ---------------------------------------------------------------------------
def pdesc(alpha=3.0, grid=(20, 24, 30), size=None):
    return _lib.TgnhPmeDesc(C.sizeof(_lib.TgnhPmeDesc) if size is None else size, (C.c_int32 * 3)(*grid), alpha)


def test_refusals_on_a_host_only_handle():
    s, table, info = system_b()
    top = HostTopology(s, integrator())
    lib = top.lib
    assert C.sizeof(_lib.TgnhPmeDesc) == 24
    assert lib.tgnh_set_nonbonded_pme(None, None) == _lib.ERR_ARG
    assert lib.tgnh_set_nonbonded_pme(top.h, C.byref(pdesc())) == _lib.ERR_STATE and "no nonbonded table" in lib.tgnh_last_error().decode()
    assert lib.tgnh_set_nonbonded_pme(top.h, None) == _lib.TGNH_OK                # nothing to clear: fine
    f = NonbondedForces(top, table)
    assert f.pme is None and f.ewald is None
    f.set_pme(2.5, 10, 12, 15)
    assert f.pme == (2.5, (10, 12, 15)) and f.ewald is None
    bad = [(pdesc(size=16), _lib.ERR_ARG, "struct_size 16"), (pdesc(alpha=0.0), _lib.ERR_ARG, "alpha is not finite or not positive"),
           (pdesc(alpha=-1.0), _lib.ERR_ARG, "alpha is not finite"), (pdesc(alpha=np.nan), _lib.ERR_ARG, "alpha is not finite"),
           (pdesc(alpha=np.inf), _lib.ERR_ARG, "alpha is not finite"), (pdesc(grid=(5, 24, 30)), _lib.ERR_ARG, "grid[0] = 5 is not in [6, 256]"),
           (pdesc(grid=(20, 24, 257)), _lib.ERR_ARG, "grid[2] = 257 is not in [6, 256]"), (pdesc(grid=(20, -4, 30)), _lib.ERR_ARG, "grid[1] = -4"),
           (pdesc(grid=(20, 14, 30)), _lib.ERR_ARG, "grid[1] = 14 has a prime factor other than 2, 3 and 5"),
           (pdesc(grid=(20, 24, 251)), _lib.ERR_ARG, "grid[2] = 251 has a prime factor")]
    for d, status, text in bad:
        assert lib.tgnh_set_nonbonded_pme(top.h, C.byref(d)) == status, text
        assert text in lib.tgnh_last_error().decode()
        assert f.pme == (2.5, (10, 12, 15))                      # a refused call leaves what was in force
    assert lib.tgnh_set_nonbonded_pme(top.h, C.byref(pdesc(grid=(256, 256, 256)))) == _lib.TGNH_OK     # 2^24 points: the most there can be
    assert f.pme == (3.0, (256, 256, 256))
    assert lib.tgnh_get_nonbonded_pme(top.h, None) == _lib.ERR_ARG
    for call in (f.ewald_energy, f.pme_grids):
        with pytest.raises(TgnhError, match="host-only") as err:
            call()
        assert err.value.status == _lib.ERR_STATE
    # one setting, two forms: each setter replaces what is in force, NULL to either goes back to the reaction field
    f.set_ewald(2.5, 1, 2, 3)
    assert f.ewald == (2.5, (1, 2, 3), 52) and f.pme is None
    f.set_pme(2.0, 6, 6, 6)
    assert f.pme == (2.0, (6, 6, 6)) and f.ewald is None
    e, m = _lib.TgnhEwaldDesc(), C.c_int(7)
    assert lib.tgnh_get_nonbonded_ewald(top.h, C.byref(e), C.byref(m)) == _lib.TGNH_OK and e.struct_size == 0 and m.value == 0
    f.clear_ewald()
    assert f.pme is None and f.ewald is None
    f.set_pme(2.0, 6, 6, 6)
    f.clear_pme()
    assert f.pme is None
    f.set_ewald(2.5, 1, 2, 3)
    f.clear_pme()
    assert f.ewald is None
    # tgnh_set_nonbonded_force drops the setting: a new table, and a clearing call
    f.set_pme(2.0, 6, 6, 6)
    f = NonbondedForces(top, table)
    assert f.pme is None
    f.set_pme(2.0, 6, 6, 6)
    f.clear()
    assert f.pme is None and f.num_terms == (0, 0, 0)
    # the explicit sum's refusal points here, and keeps its words
    f = NonbondedForces(top, table)
    d = _lib.TgnhEwaldDesc(24, (C.c_int32 * 3)(64, 64, 64), 3.0)
    assert lib.tgnh_set_nonbonded_ewald(top.h, C.byref(d)) == _lib.ERR_UNSUPPORTED
    assert "more than 2^20" in lib.tgnh_last_error().decode() and "tgnh_set_nonbonded_pme" in lib.tgnh_last_error().decode()
    top.close()


def test_more_than_2_24_points_cannot_be_asked_for():
    """every component is at most 256, so nx ny nz <= 2^24: the TGNH_ERR_UNSUPPORTED branch guards a larger PME_MAX_GRID to come"""
    assert 256 ** 3 == 2 ** 24


def test_the_ways_in():
    s, table, info = system_b()
    top = HostTopology(s, integrator())
    f = NonbondedForce()
    for row in table[3]:
        f.addParticle(*row)
    for (p1, p2), row in zip(table[4], table[5]):
        f.addException(int(p1), int(p2), *row)
    f.setCutoffDistance(1.0)
    f.setNonbondedMethod(f.CutoffPeriodic)
    # pme=True on an owner without a box: refused before any library call
    with pytest.raises(TgnhError, match="setPeriodicBoxVectors first, or pass pme=") as e:
        NonbondedForces(top, f, pme=True)
    assert e.value.status == _lib.ERR_STATE
    out = (C.c_int * 3)()
    assert top.lib.tgnh_get_num_nonbonded_terms(top.h, out) == 0 and tuple(out) == (0, 0, 0)
    with pytest.raises(TgnhError, match="two forms of one setting") as e:
        NonbondedForces(top, f, ewald=(2.5, 1, 2, 3), pme=(2.5, 10, 12, 15))
    assert e.value.status == _lib.ERR_ARG and tuple(out) == (0, 0, 0)
    nb = NonbondedForces(top, f, pme=(2.5, 10, 12, 15))
    assert nb.pme == (2.5, (10, 12, 15)) and nb.ewald is None and nb.num_terms[0] == s.num_particles
    top.setPeriodicBoxVectors((BOX_B[0], 0, 0), (0, BOX_B[1], 0), (0, 0, BOX_B[2]))
    nb = NonbondedForces(top, f, pme=True)                       # from the owner's box and the tolerance
    want = f.pme_parameters(BOX_B)
    assert nb.pme == (want[0], tuple(want[1:])) and len(set(want[1:])) == 3
    f.setPMEParameters(3.0, 20, 24, 30)
    assert NonbondedForces(top, f, pme=True).pme == (3.0, (20, 24, 30))
    f.setNonbondedMethod(f.Ewald)                                # a method-Ewald object with pme=: the mesh, not the explicit sum
    nb = NonbondedForces(top, f, pme=(2.0, 6, 6, 6))
    assert nb.pme == (2.0, (6, 6, 6)) and nb.ewald is None
    assert NonbondedForces(top, f).ewald is not None             # ... and without it the explicit sum as before
    nb = NonbondedForces(top, table, pme=(2.0, 12, 12, 12))       # a method-2 tuple
    assert nb.pme == (2.0, (12, 12, 12))
    assert NonbondedForces(top, table).pme is None
    with pytest.raises(TgnhError, match="pme: ") as e:
        NonbondedForces(top, table, pme=(2.0, 6, 6))
    assert e.value.status == _lib.ERR_ARG
    with pytest.raises(TgnhError, match="pme=True takes") as e:
        NonbondedForces(top, table, pme=True)
    assert e.value.status == _lib.ERR_ARG
    with pytest.raises(TgnhError, match="only TGNH_NB_CUTOFF_PERIODIC"):
        NonbondedForces(top, (3,) + table[1:], pme=(2.0, 6, 6, 6))
    with pytest.raises(ValueError):
        f.setNonbondedMethod(4)                                  # PME is not a method constant here
    top.close()
