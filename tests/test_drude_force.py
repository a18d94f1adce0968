"""CPU tests of the library's own DrudeForce: tgnh_set_drude_force's checks on a host-only handle, forces.DrudeForce and
DrudeSystem.set_drude_force, and the yardstick tests/test_drude_force_gpu.py measures the kernel against.

The yardstick is `evaluate` below: the terms of include/drude_tgnh.h -- the isotropic spring, the two anisotropy axes, the four site
pairs of a screened pair -- over arrays of any floating type.  Run on numpy longdouble (fp80) it is THE REFERENCE; run on float64 it
is THE TWIN, whose every operation numpy rounds on its own, in the order written -- what the device is asked to reproduce bit for bit
for the isotropic shares.  The constants k1, k2, k3, a, K are formed in fp64 from include/drude_tgnh.h's formulas, as the library forms them,
and handed to both.  The reference is itself checked here: its forces against central finite differences of its own energy in fp80.

The table and the states of the GPU tests are built HERE (`drude_system`, `state`), once, and never changed: 9 "ring" molecules --
four polarizable atoms h0..h3 with their Drude particles and one plain atom; h0's row has both axes (p2 = h1, p3 = h2, p4 = h3),
h1's the first only (p2 = h0), h2's and h3's the second only (p3, p4 among h0, h1), so h0 is the parent of its own row, p2, p3 and p4
of its neighbours' and a member of two screened pairs --, 31 three-slot waters (O, D, H: one isotropic row) and 15 lone ions:
189 slots (padded 192), 67 rows in shuffled order, 134 receiving slots, 55 slots in no term; screened pairs inside the rings, between
rings and waters more than a wavefront of slots apart, one of them with thole = 0.  Drude particles 0.005-0.02 nm off their parents;
molecule centres on a 0.6 nm lattice; the states split into the stored types as Context::setPositions does.

THE GPU MARGIN.  Per term (a spring of a row, or one site pair of a screened pair), the largest difference between twin and
reference over the term's share components, relative to the largest share component of that term in the reference, over the three
states, isotropic springs left out (they are compared bit for bit): measured by test_the_margin_between_twin_and_reference at
5.16e-15 -- an axis spring whose delta is nearly along its axis: delta - s e cancels and keeps the roundings of s e; the site pairs
stay below 1e-15.  MEASURED_MARGIN is that figure rounded up, 5.2e-15; the GPU gate is GATE = 16 x MEASURED_MARGIN = 8.3e-14: room
for another order of operations, another exp and for contraction (the factor and the reason of tests/test_virtual_sites.py).  The
energies' margin is measured beside it (relative to the sum of |term energies|: 1.6e-16) and lies below it.  It comes from the
reference and the number format, never from the device."""
import numpy as np
import pytest

from openmm_drudenose_amd import _lib
from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator, HostTopology, TgnhError
from openmm_drudenose_amd.forces import DrudeForce
from openmm_drudenose_amd.system import DrudeSystem

PRECISIONS = ("double", "mixed", "single")
ONE_4PI_EPS0 = 138.935456
FIXED = 4294967296.0
MEASURED_MARGIN = 5.2e-15
GATE = 16 * MEASURED_MARGIN
RINGS, WATERS, IONS = 9, 31, 15
L = np.longdouble
_cache = {}


# ---------------------------------------------------------------------------
# the terms, over arrays [T, 3] of one floating type
# ---------------------------------------------------------------------------
def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])[:, None]


def _axis(k, d, delta):
    """-> f1, f2, E of one anisotropic spring along d"""
    ln = np.sqrt(_dot(d, d))
    e = d / ln
    s = _dot(e, delta)
    ks = k * s
    return ks * e, (ks / ln) * (delta - s * e), ((k.dtype.type(0.5) * ks) * s)[:, 0]


def _site_pair(a, sk, delta):
    """-> the share of `first` (delta = x(first) - x(second)) and E of one screened site pair"""
    one, half = a.dtype.type(1), a.dtype.type(0.5)
    r2 = _dot(delta, delta)
    r = np.sqrt(r2)
    u = a * r
    ex = np.exp(-u)
    S = one - (one + half * u) * ex
    c = (sk * (S / r - ((half * (one + u)) * ex) * a)) / r2
    return c * delta, ((sk * S) / r)[:, 0]


def constants(particles, params, screened, thole):
    """k1, k2, k3 [n] and a, K [m] in fp64, from the formulas of include/drude_tgnh.h"""
    q, alpha = params[:, 0], params[:, 1]
    has12, has34 = particles[:, 2] != -1, (particles[:, 3] != -1) & (particles[:, 4] != -1)
    a1, a2 = np.where(has12, params[:, 2], 1.0), np.where(has34, params[:, 3], 1.0)
    a3 = 3.0 - a1 - a2
    cq2 = ONE_4PI_EPS0 * q * q
    k3 = cq2 / (alpha * a3)
    k1 = np.where(has12, cq2 / (alpha * a1) - k3, 0.0)
    k2 = np.where(has34, cq2 / (alpha * a2) - k3, 0.0)
    i, j = screened[:, 0], screened[:, 1]
    a = thole / (alpha[i] * alpha[j]) ** (1.0 / 6.0)
    K = ONE_4PI_EPS0 * q[i] * q[j]
    return k1, k2, k3, a, K


def evaluate(tables, x, dtype):
    """Every term of a table in `dtype` -> list of terms (name, slots: list of index arrays [T], shares: list of [T, 3] beside them,
    energy [T], screened: bool), one entry per kind of term, T the rows or pairs that have it."""
    particles, params, screened, thole = tables
    k1, k2, k3, a, K = [v.astype(dtype)[:, None] for v in constants(*tables)]
    x = x.astype(dtype)
    P, P1, P2, P3, P4 = particles.T
    out = []
    delta = x[P] - x[P1]
    t = k3 * delta
    out.append(("isotropic", [P, P1], [-t, t], ((dtype(0.5) * k3) * _dot(delta, delta))[:, 0], False))
    m = np.flatnonzero(P2 != -1)
    f1, f2, e = _axis(k1[m], x[P1[m]] - x[P2[m]], delta[m])
    out.append(("axis 12", [P[m], P1[m], P2[m]], [-f1, f1 - f2, f2], e, False))
    m = np.flatnonzero(P3 != -1)
    f1, f2, e = _axis(k2[m], x[P3[m]] - x[P4[m]], delta[m])
    out.append(("axis 34", [P[m], P1[m], P3[m], P4[m]], [-f1, f1, -f2, f2], e, False))
    i, j = screened[:, 0], screened[:, 1]
    for fi, first in enumerate((P[i], P1[i])):                   # Drude_i-Drude_j, Drude_i-parent_j, parent_i-Drude_j, parent_i-parent_j
        for si, second in enumerate((P[j], P1[j])):
            v, e = _site_pair(a, K if fi == si else -K, x[first] - x[second])
            out.append((f"site pair {fi}{si}", [first, second], [v, -v], e, True))
    return out


def total_forces(terms, n, dtype):
    f = np.zeros((n, 3), dtype)
    for _, slots, shares, _, _ in terms:
        for s, v in zip(slots, shares):
            np.add.at(f, s, v)
    return f


def energies(terms):
    """-> (springs, screened pairs): plain sums in the terms' type"""
    return (sum(e.sum() for _, _, _, e, scr in terms if not scr), sum(e.sum() for _, _, _, e, scr in terms if scr))


# ---------------------------------------------------------------------------
# the table and the states of the GPU tests
# ---------------------------------------------------------------------------
RING = np.array([[0.0, 0.0, 0.0], [0.14, 0.0, 0.01], [-0.05, 0.13, 0.0], [-0.04, -0.07, 0.12], [0.09, 0.1, -0.1]])     # h0..h3, the plain atom


def drude_system():
    """-> (DrudeSystem with positions and the DrudeForce attached, tables): the table of the module docstring"""
    if "system" in _cache:
        return _cache["system"]
    rng = np.random.default_rng(20250907)
    mass, pos, resid, rows = [], [], [], []              # rows: (p, p1, p2, p3, p4, q, alpha, a12, a34)
    n, mol = 0, 0
    cells = rng.permutation(5 * 5 * 5)[:RINGS + WATERS + IONS]
    centre = lambda c: (np.array([c // 25, (c // 5) % 5, c % 5]) - 2.0) * 0.6                     # noqa: E731
    kinds = ["ring"] * RINGS + ["water"] * WATERS + ["ion"] * IONS
    order = rng.permutation(len(kinds))                          # molecules of the three kinds interleaved
    ring_rows, water_rows = [], []

    def drude(parent):
        d = rng.normal(size=3)
        return parent + d / np.linalg.norm(d) * rng.uniform(0.005, 0.02)
    for c, which in zip(cells, [kinds[o] for o in order]):
        rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        if which == "ring":                                      # slots h0 d0 h1 d1 h2 d2 h3 d3 c
            g = RING @ rot.T + centre(c)
            h = [n, n + 2, n + 4, n + 6]
            for a in range(4):
                pos += [g[a], drude(g[a])]
                mass += [12.011 - 0.4, 0.4]
            pos.append(g[4]); mass.append(1.008)
            alpha = rng.uniform(0.0008, 0.0016, 4)
            q = -rng.uniform(1.0, 2.0, 4)
            ring_rows.append(len(rows))
            rows += [(h[0] + 1, h[0], h[1], h[2], h[3], q[0], alpha[0], rng.uniform(0.8, 1.1), rng.uniform(0.9, 1.2)),
                     (h[1] + 1, h[1], h[0], -1, -1, q[1], alpha[1], rng.uniform(0.7, 1.3), 7.0),              # (aniso34 is not read)
                     (h[2] + 1, h[2], -1, h[0], h[1], q[2], alpha[2], -3.0, rng.uniform(0.7, 1.3)),           # (aniso12 is not read)
                     (h[3] + 1, h[3], -1, h[1], h[0], q[3], alpha[3], 0.0, rng.uniform(0.7, 1.3))]
            resid += [mol] * 9; n += 9
        elif which == "water":                                   # O D H
            g = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.09572, 0.0, 0.0]]) @ rot.T + centre(c)
            g[1] = drude(g[0])
            pos += list(g); mass += [15.9994 - 0.4, 0.4, 1.008]
            water_rows.append(len(rows))
            rows.append((n + 1, n, -1, -1, -1, -1.71636, 0.00097825, 0.0, 0.0))
            resid += [mol] * 3; n += 3
        else:
            pos.append(centre(c)); mass.append(22.99); resid.append(mol); n += 1
        mol += 1
    shuffle = rng.permutation(len(rows))                         # row k is pair k: the pairs in an order that is not the slots'
    new_of = np.argsort(shuffle)
    rows = [rows[o] for o in shuffle]
    force = DrudeForce()
    for r in rows:
        force.addParticle(*r)
    rr, wr = [new_of[np.array(ring_rows) + a] for a in range(4)], new_of[np.array(water_rows)]
    for m in range(RINGS):
        force.addScreenedPair(rr[0][m], rr[1][m], 1.3 + 0.01 * m)
        force.addScreenedPair(rr[2][m], rr[0][m], 2.6)                       # (h0's row second)
        force.addScreenedPair(rr[1][m], rr[3][m], 0.0 if m == 4 else 1.1)    # one pair with thole = 0
    slot_of_row = np.array([r[0] for r in rows])
    far = 0
    for m in range(RINGS):                                       # between a ring and waters more than a wavefront of slots away
        for w in wr:
            if abs(slot_of_row[w] - slot_of_row[rr[0][m]]) > 64 and far < 2 * (m + 1):
                pair = (w, rr[m % 4][m]) if far % 2 else (rr[m % 4][m], w)          # the water's row first, then second
                force.addScreenedPair(pair[0], pair[1], 0.9 + 0.1 * far)
                far += 1
    pos = np.array(pos)
    tables = force.tables()
    s = DrudeSystem(mass=np.array(mass), pair_drude=tables[0][:, 0].copy(), pair_parent=tables[0][:, 1].copy(), resid=np.array(resid, np.int32),
                    positions=pos, velocities=np.zeros_like(pos), name="9 rings, 31 waters, 15 ions: 67 rows")
    s.set_drude_force(force)
    for a in tables:
        a.setflags(write=False)
    _cache["system"] = (s, tables)
    return _cache["system"]


def state(precision):
    """The stored arrays of the system in a precision and their fp64 reading -> dict: posq [N, 3] (float32 / float64), corr [N, 3]
    float32 or None, x: the positions as the device reads them (fp64).  Built once; callers copy what they change."""
    key = ("state", precision)
    if key not in _cache:
        x = drude_system()[0].positions
        real = np.float64 if precision == "double" else np.float32
        posq = x.astype(real)
        corr = (x - posq.astype(np.float64)).astype(np.float32) if precision == "mixed" else None
        st = dict(posq=posq, corr=corr)
        st["x"] = posq.astype(np.float64) + (corr.astype(np.float64) if corr is not None else 0.0)
        for a in st.values():
            if a is not None:
                a.setflags(write=False)
        _cache[key] = st
    return _cache[key]


def results(precision, dtype):
    """evaluate() on a state, computed once per (precision, type)"""
    key = ("results", precision, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = evaluate(drude_system()[1], state(precision)["x"], dtype)
    return _cache[key]


def integrator():
    return DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)


def receivers(tables):
    particles = tables[0]                                         # (a screened pair's sites receive through their own rows already)
    return np.unique(particles[particles >= 0])


# ---------------------------------------------------------------------------
# the table is what the GPU tests need it to be
# ---------------------------------------------------------------------------
def test_the_table_has_the_shapes_the_kernel_can_go_wrong_at():
    s, tables = drude_system()
    particles, params, screened, thole = tables
    n = s.num_particles
    assert n == 189 and n % 32 != 0 and len(particles) == 67 and len(particles) % 64 != 0
    recv = receivers(tables)
    assert len(recv) > 128 and len(recv) < n                                                   # a third wavefront; slots in no term
    has12, has34 = particles[:, 2] != -1, particles[:, 3] != -1
    assert all(np.any(has12 == x) and np.any(has34[has12 == x] == y) for x in (False, True) for y in (False, True))      # the four shapes
    assert np.any(np.diff(particles[:, 0]) < 0)                                                # rows not in slot order
    i, j = screened[:, 0], screened[:, 1]
    same_mol = s.resid[particles[i, 0]] == s.resid[particles[j, 0]]
    assert same_mol.any() and np.any(~same_mol & (np.abs(particles[i, 0] // 64 - particles[j, 0] // 64) >= 1))
    assert np.count_nonzero(thole == 0.0) == 1
    # a slot with >= 6 entries: the parent of its own row, p2, p3 and p4 of its neighbours', in two screened pairs
    entries = np.bincount(particles[particles >= 0], minlength=n)
    for col in (0, 1):
        np.add.at(entries, particles[i, col], 1); np.add.at(entries, particles[j, col], 1)
    busy = [h for h in particles[:, 1] if h in particles[:, 2] and h in particles[:, 3] and h in particles[:, 4]]
    assert busy and all(entries[h] >= 6 for h in busy)
    pair_rows = np.concatenate([i, j])
    assert all(np.count_nonzero(particles[pair_rows, 1] == h) >= 2 for h in busy)
    for precision in PRECISIONS:
        st = state(precision)
        d = np.linalg.norm(st["x"][particles[:, 0]] - st["x"][particles[:, 1]], axis=1)
        assert 0.0049 < d.min() and d.max() < 0.0201
        if precision == "mixed":
            assert np.count_nonzero(st["corr"]) > 0.8 * st["corr"].size
    k1, k2, k3, a, K = constants(*tables)
    assert k3.min() > 0 and np.all(k1[~has12] == 0) and np.all(k2[~has34] == 0) and np.any(k1 < 0) and np.any(k1 > 0)


# ---------------------------------------------------------------------------
# the reference checked against itself, the twin against numpy, the margin
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forces_against_finite_differences_of_the_energy(precision):
    """-dE/dx by central differences in fp80, h = 1e-6 nm.  Truncation: h^2 / 6 x the third derivative -- a site pair at 0.14 nm,
    6 K / r^4 = 3e6, gives 5e-7 kJ/mol/nm; an axis spring k delta / |d|^2 = 3e5 x 0.02 / 0.02 gives as much -- against forces of
    6e3 kJ/mol/nm: 1e-10 of the largest component.  Rounding: 2^-64 x 1e3 kJ/mol / 2e-6 nm = 3e-11 of it.  Asked for: 1e-8."""
    s, tables = drude_system()
    x = state(precision)["x"].astype(L)
    f = total_forces(results(precision, L), s.num_particles, L)
    h = L(1e-6)
    worst = 0.0
    for i in receivers(tables):
        for c in range(3):
            up, dn = x.copy(), x.copy()
            up[i, c] += h; dn[i, c] -= h
            eu, ed = sum(energies(evaluate(tables, up, L))), sum(energies(evaluate(tables, dn, L)))
            worst = max(worst, float(abs(-(eu - ed) / (2 * h) - f[i, c])))
    scale = float(np.abs(f).max())
    print(f"forces against central differences, {precision}: {worst:.2e} of a largest component {scale:.2e}")
    assert worst <= 1e-8 * scale
    assert np.abs(f.sum(0)).max() <= 2.0 ** -52 * scale                                 # every term's shares add up to zero


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_twins_isotropic_shares_are_three_lines_of_numpy(precision):
    s, tables = drude_system()
    particles, params = tables[0], tables[1]
    x = state(precision)["x"]
    k3 = ONE_4PI_EPS0 * params[:, 0] * params[:, 0] / (params[:, 1] * (3.0 - np.where(particles[:, 2] != -1, params[:, 2], 1.0) - np.where(particles[:, 3] != -1, params[:, 3], 1.0)))
    t = k3[:, None] * (x[particles[:, 0]] - x[particles[:, 1]])
    name, slots, shares, _, _ = results(precision, np.float64)[0]
    assert name == "isotropic" and np.array_equal(slots[0], particles[:, 0]) and np.array_equal(slots[1], particles[:, 1])
    assert np.array_equal(shares[0].view(np.uint64), (-t).view(np.uint64)) and np.array_equal(shares[1].view(np.uint64), t.view(np.uint64))


def margins():
    """-> (shares, energies): the largest difference between twin and reference per term over the term's largest share component
    (isotropic springs left out), and of the two energies over the sum of |term energies|, over the three states"""
    worst, worst_e = 0.0, 0.0
    for precision in PRECISIONS:
        ref, twin = results(precision, L), results(precision, np.float64)
        for (name, _, rs, re, _), (_, _, ts, te, _) in zip(ref, twin):
            scale = np.max([np.abs(v).max(1) for v in rs], axis=0)
            d = np.max([np.abs(t.astype(L) - r).max(1) for r, t in zip(rs, ts)], axis=0)
            ok = scale > 0                                       # (the pair with thole = 0: shares of exactly 0 in both)
            assert np.all(d[~ok] == 0)
            if name != "isotropic" and ok.any():
                worst = max(worst, float((d[ok] / scale[ok]).max()))
        for scr in (False, True):
            tot = sum(np.abs(e).sum() for _, _, _, e, sc in ref if sc == scr)
            diff = abs(L(energies(twin)[scr]) - energies(ref)[scr])
            worst_e = max(worst_e, float(diff / tot))
    return worst, worst_e


def test_the_margin_between_twin_and_reference():
    """MEASURED_MARGIN of the module docstring, measured: it must cover the figure, and not by more than a quarter."""
    figure, energy = margins()
    print(f"fp64 twin against the fp80 reference: shares {figure:.3e} of the term's largest share component, energies {energy:.3e} of the sum of "
          f"|term energies|; MEASURED_MARGIN {MEASURED_MARGIN:.2e}, the GPU gate {GATE:.2e}")
    assert 0.75 * MEASURED_MARGIN <= figure <= MEASURED_MARGIN
    assert energy <= MEASURED_MARGIN


def test_a_thole_of_zero_contributes_exactly_nothing():
    s, tables = drude_system()
    m = int(np.flatnonzero(tables[3] == 0.0)[0])
    for dtype in (np.float64, L):
        for name, _, shares, e, scr in results("mixed", dtype):
            if scr:
                assert e[m] == 0 and all(np.all(v[m] == 0) for v in shares)


# ---------------------------------------------------------------------------
# tgnh_set_drude_force on a host-only handle
# ---------------------------------------------------------------------------
def host(s):
    return HostTopology(s, integrator())


def refused(top, tables, match):
    before = top.num_drude_force_terms
    with pytest.raises(TgnhError, match=match) as e:
        top.set_drude_force(tables)
    assert e.value.status == _lib.ERR_ARG
    assert top.num_drude_force_terms == before                                              # a refused table changes nothing


def test_accepted_tables_and_the_counts():
    s, tables = drude_system()
    top = host(s)
    assert top.num_drude_force_terms == (0, 0)
    top.set_drude_force(tables)
    assert top.num_drude_force_terms == (67, len(tables[2]))
    top.set_drude_force((tables[0], tables[1], tables[2][:3], tables[3][:3]))              # a second table replaces the first
    assert top.num_drude_force_terms == (67, 3)
    top.set_drude_force(s.drude_force)                                                      # the object itself
    assert top.num_drude_force_terms == (67, len(tables[2]))
    top.set_drude_force(None)                                                               # n = 0 clears it
    assert top.num_drude_force_terms == (0, 0)
    # the launching calls on a host-only handle
    out = np.zeros(2)
    assert top.lib.tgnh_compute_drude_force(top.h, None, 0, None) == _lib.ERR_STATE
    assert top.lib.tgnh_get_drude_energy(top.h, None, out.ctypes.data_as(_lib.c_f64p)) == _lib.ERR_STATE
    assert top.lib.tgnh_get_num_drude_force_terms(top.h, None, None) == _lib.ERR_ARG
    assert top.lib.tgnh_set_drude_force(None, 0, None, None, 0, None, None) == _lib.ERR_ARG
    top.close()


def test_refusals():
    s, tables = drude_system()
    particles, params, screened, thole = [a.copy() for a in tables]
    n = s.num_particles
    top = host(s)
    lib = top.lib
    i32, f64 = lambda v: v.ctypes.data_as(_lib.c_i32p), lambda v: v.ctypes.data_as(_lib.c_f64p)
    both = int(np.flatnonzero((particles[:, 2] != -1) & (particles[:, 3] != -1))[0])
    only12 = int(np.flatnonzero((particles[:, 2] != -1) & (particles[:, 3] == -1))[0])
    only34 = int(np.flatnonzero((particles[:, 2] == -1) & (particles[:, 3] != -1))[0])
    iso = int(np.flatnonzero((particles[:, 2] == -1) & (particles[:, 3] == -1))[0])

    def with_(pa=None, pr=None, sc=None, th=None):
        p2, q2, s2, t2 = particles.copy(), params.copy(), screened.copy(), thole.copy()
        if pa is not None:
            p2[pa[0], pa[1]] = pa[2]
        if pr is not None:
            q2[pr[0], pr[1]] = pr[2]
        if sc is not None:
            s2[sc[0], sc[1]] = sc[2]
        if th is not None:
            t2[th[0]] = th[1]
        return p2, q2, s2, t2
    for trial in (0, 1):                                         # on an empty table, then on one in force
        before = top.num_drude_force_terms
        for count in (1, 66, 68, -1):
            assert lib.tgnh_set_drude_force(top.h, count, i32(particles), f64(params), 0, None, None) == _lib.ERR_ARG
        assert lib.tgnh_set_drude_force(top.h, 67, None, f64(params), 0, None, None) == _lib.ERR_ARG
        assert lib.tgnh_set_drude_force(top.h, 67, i32(particles), None, 0, None, None) == _lib.ERR_ARG
        assert lib.tgnh_set_drude_force(top.h, 67, i32(particles), f64(params), 1, None, f64(thole)) == _lib.ERR_ARG
        assert lib.tgnh_set_drude_force(top.h, 67, i32(particles), f64(params), 1, i32(screened), None) == _lib.ERR_ARG
        assert lib.tgnh_set_drude_force(top.h, 67, i32(particles), f64(params), -1, i32(screened), f64(thole)) == _lib.ERR_ARG
        assert top.num_drude_force_terms == before
        refused(top, with_(pa=(5, 0, particles[5, 1])), "row 5 names")                       # row k is not pair k
        refused(top, with_(pa=(5, 1, particles[6, 1])), "row 5 names")
        swapped = particles.copy(); swapped[[3, 4]] = swapped[[4, 3]]
        refused(top, (swapped, params, screened, thole), "row 3 names")
        refused(top, with_(pa=(both, 2, n)), "row %d: index %d out of range" % (both, n))
        refused(top, with_(pa=(both, 3, -2)), "row %d: index -2 out of range" % both)
        refused(top, with_(pa=(both, 4, n + 7)), "row %d: index %d out of range" % (both, n + 7))
        refused(top, with_(pa=(only12, 2, particles[only12, 0])), "row %d: p2 is p or p1" % only12)
        refused(top, with_(pa=(only12, 2, particles[only12, 1])), "row %d: p2 is p or p1" % only12)
        refused(top, with_(pa=(only34, 3, particles[only34, 4])), "row %d: p3 is p4" % only34)
        refused(top, with_(pa=(only34, 3, -1)), "row %d: exactly one of p3 and p4" % only34)
        refused(top, with_(pa=(iso, 4, 0)), "row %d: exactly one of p3 and p4" % iso)
        for bad in (np.nan, np.inf):
            refused(top, with_(pr=(iso, 0, bad)), "row %d: the charge is not finite" % iso)
        for bad in (np.nan, np.inf, 0.0, -0.001):
            refused(top, with_(pr=(iso, 1, bad)), "row %d: the polarizability" % iso)
            refused(top, with_(pr=(only12, 2, bad)), "row %d: aniso12" % only12)
            refused(top, with_(pr=(both, 3, bad)), "row %d: aniso34" % both)
        refused(top, with_(pr=(only12, 2, 2.0)), "row %d: 3 - aniso12 - aniso34 is not positive" % only12)
        refused(top, with_(pr=(both, 3, 3.0 - params[both, 2])), "row %d: 3 - aniso12" % both)
        top.set_drude_force(with_(pr=(iso, 2, np.nan)))                                      # an aniso value the row does not read may be anything
        top.set_drude_force(with_(pr=(only12, 3, -1.0)))
        refused(top, with_(sc=(2, 0, 67)), "screened pair 2: row 67 out of range")
        refused(top, with_(sc=(2, 1, -1)), "screened pair 2: row -1 out of range")
        refused(top, with_(sc=(4, 1, screened[4, 0])), "screened pair 4 names row %d twice" % screened[4, 0])
        dup = screened.copy(); dup[7] = dup[1]
        refused(top, (particles, params, dup, thole), "screened pair 7: rows .* are listed twice")
        dup[7] = dup[1][::-1]
        refused(top, (particles, params, dup, thole), "screened pair 7: rows .* are listed twice")                       # ... in the other order
        for bad in (-0.5, np.nan, np.inf):
            refused(top, with_(th=(3, bad)), "screened pair 3: thole")
        with pytest.raises(TgnhError, match="one row of four parameters"):
            top.set_drude_force((particles, params[:5], screened, thole))
        top.set_drude_force(tables)
        assert top.num_drude_force_terms == (67, len(screened))
    top.close()
    plain = DrudeSystem(mass=np.ones(4), pair_drude=np.zeros(0, np.int32), pair_parent=np.zeros(0, np.int32), resid=np.zeros(4, np.int32))
    top = host(plain)                                            # a system without pairs takes the empty table only
    top.set_drude_force(DrudeForce())
    assert lib.tgnh_set_drude_force(top.h, 1, i32(particles), f64(params), 0, None, None) == _lib.ERR_ARG
    top.close()


# ---------------------------------------------------------------------------
# forces.DrudeForce and DrudeSystem.set_drude_force
# ---------------------------------------------------------------------------
def test_the_force_object_round_trips_its_parameters():
    f = DrudeForce()
    assert f.getNumParticles() == 0 and f.getNumScreenedPairs() == 0
    assert f.addParticle(1, 0, -1, -1, -1, -1.5, 0.001) == 0
    assert f.addParticle(3, 2, 0, 4, 5, -1.25, 0.0012, 0.9, 1.05) == 1
    assert f.getParticleParameters(0) == (1, 0, -1, -1, -1, -1.5, 0.001, 0.0, 0.0)
    assert f.getParticleParameters(1) == (3, 2, 0, 4, 5, -1.25, 0.0012, 0.9, 1.05)
    f.setParticleParameters(0, 1, 0, 2, -1, -1, -1.75, 0.002, 1.1, 0.0)
    assert f.getParticleParameters(0) == (1, 0, 2, -1, -1, -1.75, 0.002, 1.1, 0.0)
    assert f.addScreenedPair(0, 1, 2.6) == 0 and f.getScreenedPairParameters(0) == (0, 1, 2.6)
    f.setScreenedPairParameters(0, 1, 0, 1.3)
    assert f.getScreenedPairParameters(0) == (1, 0, 1.3) and f.getNumParticles() == 2 and f.getNumScreenedPairs() == 1
    for bad in (-1, 2):
        with pytest.raises(IndexError):
            f.getParticleParameters(bad)
    with pytest.raises(IndexError):
        f.setScreenedPairParameters(1, 0, 1, 1.0)
    particles, params, screened, thole = f.tables()
    assert particles.dtype == np.int32 and particles.tolist() == [[1, 0, 2, -1, -1], [3, 2, 0, 4, 5]]
    assert params.dtype == np.float64 and params.tolist() == [[-1.75, 0.002, 1.1, 0.0], [-1.25, 0.0012, 0.9, 1.05]]
    assert screened.dtype == np.int32 and screened.tolist() == [[1, 0]] and thole.tolist() == [1.3]
    e = DrudeForce().tables()
    assert [a.shape for a in e] == [(0, 5), (0, 4), (0, 2), (0,)]


def test_the_system_refuses_a_row_that_is_not_its_pair():
    s, tables = drude_system()
    t = DrudeSystem(mass=s.mass, pair_drude=s.pair_drude, pair_parent=s.pair_parent, resid=s.resid)
    assert t.drude_force is None
    good = s.drude_force
    t.set_drude_force(good)
    assert t.drude_force is good
    bad = DrudeForce()
    for k in range(good.getNumParticles()):
        row = list(good.getParticleParameters(k))
        if k == 11:
            row[1] = int(s.pair_parent[12])
        bad.addParticle(*row)
    with pytest.raises(ValueError, match="row 11 names"):
        t.set_drude_force(bad)
    short = DrudeForce()
    short.addParticle(*good.getParticleParameters(0))
    with pytest.raises(ValueError, match="1 rows for 67 Drude pairs"):
        t.set_drude_force(short)
    assert t.drude_force is good
    t.set_drude_force(None)
    assert t.drude_force is None
