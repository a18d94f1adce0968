"""CPU tests of the library's bonded forces: tgnh_set_bonded_forces' checks on a host-only handle, the three table classes and
BondedForces of openmm_drudenose_amd/forces.py, and the yardstick tests/test_bonded_forces_gpu.py measures the kernel against.

The yardstick is `evaluate` below: the terms of include/drude_tgnh.h -- harmonic bond, harmonic angle, periodic torsion -- over
arrays of any floating type.  Run on numpy longdouble (fp80) it is THE REFERENCE; run on float64 it is THE TWIN, whose every
operation numpy rounds on its own, in the order written (the angle through np.arctan2) -- what the device is asked to reproduce bit
for bit for the bond shares.  cos and sin of the phases are formed in fp64, as the library forms them at set time, and handed to
both.  The reference is itself checked here: its forces against central finite differences of its own energy in fp80, per term.

The tables and the states of the GPU tests are built HERE (`bonded_system`, `state`), once, and never changed: 58 branched
eight-atom chains (bonds 0-1, 1-2, 2-3, 3-4, 4-5, 2-6, 2-7: atom 2 is in 4 bonds, 8 angles and 9 torsions, three of them on the
same four atoms with n = 1, 2, 3; atoms 1, 3 and 6 carry Drude particles, 11 slots a chain), 20 three-slot waters (two bonds, one
angle) and 24 ions: two pairs of them bonded, one pair more than a work-group of slots apart; one pair on a bond with k = 0; three
in an angle with k = 0; three exactly collinear, on coordinates that every stored type holds exactly, in an angle with theta0 = pi;
twelve in no term.  722 slots (padded 736), 536 of them receive: three work-groups.  The rows of all three tables are shuffled.
Three states: the lattice (molecules on a 0.8 nm lattice, rigidly rotated), a thermal displacement (normal, 0.004 nm a component)
and a stretched one (every molecule scaled by 1.25 about its first atom, plus 0.008 nm), split into the stored types as
Context::setPositions does.  Angles stay within [50, 170] degrees and |sin| of the bond angles inside torsions above 0.3 in all.

THE GPU MARGIN.  Per term, the largest difference between twin and reference over its share components, relative to the term's
UNCANCELLED scale -- k max(r, r0) for a bond; k max(theta, theta0) / min(|a|, |b|) for an angle; k n l / min(c0.c0, c1.c1) x
max(|c0|, |c1|) for a torsion --, so that a term near its equilibrium does not inflate the figure; over the three states and the
three stored types.  Measured by test_the_margin_between_twin_and_reference at 1.83e-15 (a torsion; bonds 1.8e-16, angles 3.0e-16);
MEASURED_MARGIN is that figure rounded up, 1.9e-15, and the GPU gate is GATE = 16 x MEASURED_MARGIN = 3.0e-14: room for another order of operations, another atan2 and for contraction (the factor and the
reason of tests/test_virtual_sites.py).  The energies' margin is measured beside it (relative to the sum of |term energies|: 6.4e-16) and
lies below it.  Both come from the reference and the number format, never from the device."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import _lib
from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator, HostTopology, TgnhError
from openmm_drudenose_amd.forces import BondedForces, DrudeForce, HarmonicAngleForce, HarmonicBondForce, PeriodicTorsionForce
from openmm_drudenose_amd.system import DrudeSystem

PRECISIONS = ("double", "mixed", "single")
STATES = ("lattice", "thermal", "stretched")
KINDS = ("bond", "angle", "torsion")
FIXED = 4294967296.0
BLOCK = 256                      # csrc/tgnh_internal.h
MEASURED_MARGIN = 1.9e-15
GATE = 16 * MEASURED_MARGIN
CHAINS, WATERS, IONS = 58, 20, 24
L = np.longdouble
_cache = {}


# ---------------------------------------------------------------------------
# the terms, over arrays [T, 3] of one floating type
# ---------------------------------------------------------------------------
def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])[:, None]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def bond_terms(x1, x2, r0, k):
    """-> shares [p1, p2], E [T], scale [T]"""
    half = k.dtype.type(0.5)
    d = x2 - x1
    r = np.sqrt(_dot(d, d))
    c = (k * (r - r0)) / r
    f = c * d
    return [f, -f], (((half * k) * (r - r0)) * (r - r0))[:, 0], (np.abs(k) * np.maximum(r, r0))[:, 0]


def angle_terms(x1, x2, x3, t0, k):
    """-> shares [p1, p2, p3], E, scale, theta [T]"""
    half = k.dtype.type(0.5)
    a, b = x1 - x2, x3 - x2
    c = _cross(a, b)
    ln = np.sqrt(_dot(c, c))
    s = np.maximum(ln, k.dtype.type(1e-6))
    theta = np.arctan2(ln, _dot(a, b))
    g = k * (theta - t0)
    f1 = (g / (_dot(a, a) * s)) * _cross(c, a)
    f3 = (g / (_dot(b, b) * s)) * _cross(b, c)
    scale = np.abs(k) * np.maximum(theta, t0) / np.sqrt(np.minimum(_dot(a, a), _dot(b, b)))
    return [f1, -(f1 + f3), f3], ((half * g) * (theta - t0))[:, 0], scale[:, 0], theta[:, 0]


def torsion_terms(x1, x2, x3, x4, n, cos0, sin0, k):
    """-> shares [p1..p4], E, scale, (cos phi, sin phi) [T]; n [T] integers, cos0, sin0: of the phase"""
    one = k.dtype.type(1)
    v0, v1, v2 = x1 - x2, x3 - x2, x3 - x4
    c0, c1 = _cross(v0, v1), _cross(v1, v2)
    l2 = _dot(v1, v1)
    ln = np.sqrt(l2)
    X, Y = _dot(c0, c1), ln * _dot(v0, c1)
    hyp = np.sqrt(X * X + Y * Y)
    cp, sp = X / hyp, Y / hyp
    Cn, Sn = cp.copy(), sp.copy()
    for m in range(1, int(n.max()) if len(n) else 1):
        more = (m < n)[:, None]
        Cn, Sn = np.where(more, Cn * cp - Sn * sp, Cn), np.where(more, Sn * cp + Cn * sp, Sn)
    nn = n.astype(k.dtype)[:, None]
    e = k * (one + (Cn * cos0 + Sn * sin0))
    g = -(k * nn) * (Sn * cos0 - Cn * sin0)
    cc0, cc1 = _dot(c0, c0), _dot(c1, c1)
    f1 = ((-g * ln) / cc0) * c0
    f4 = ((g * ln) / cc1) * c1
    s = (_dot(v0, v1) / l2) * f1 - (_dot(v2, v1) / l2) * f4
    scale = np.abs(k) * nn * ln / np.minimum(cc0, cc1) * np.sqrt(np.maximum(cc0, cc1))
    return [f1, s - f1, -s - f4, f4], e[:, 0], scale[:, 0], (cp[:, 0], sp[:, 0])


def _columns(params, dtype):
    return [params[:, m].astype(dtype)[:, None] for m in range(params.shape[1])]


def evaluate(tables, x, dtype):
    """Every term of the three tables in `dtype` -> one entry per kind, in KINDS' order: (kind, slots: list of index arrays [T],
    shares: list of [T, 3] beside them, energy [T], scale [T])"""
    (bp, bpar), (ap, apar), (tp, tn, tpar) = tables
    x = x.astype(dtype)
    out = []
    sh, e, sc = bond_terms(x[bp[:, 0]], x[bp[:, 1]], *_columns(bpar, dtype))
    out.append(("bond", list(bp.T), sh, e, sc))
    sh, e, sc, _ = angle_terms(x[ap[:, 0]], x[ap[:, 1]], x[ap[:, 2]], *_columns(apar, dtype))
    out.append(("angle", list(ap.T), sh, e, sc))
    cos0, sin0 = np.cos(tpar[:, 0]).astype(dtype)[:, None], np.sin(tpar[:, 0]).astype(dtype)[:, None]      # fp64, as the library forms them
    sh, e, sc, _ = torsion_terms(x[tp[:, 0]], x[tp[:, 1]], x[tp[:, 2]], x[tp[:, 3]], tn, cos0, sin0, tpar[:, 1].astype(dtype)[:, None])
    out.append(("torsion", list(tp.T), sh, e, sc))
    return out


def total_forces(terms, n, dtype):
    f = np.zeros((n, 3), dtype)
    for _, slots, shares, _, _ in terms:
        for s, v in zip(slots, shares):
            np.add.at(f, s, v)
    return f


def energies(terms):
    """-> (bonds, angles, torsions): plain sums in the terms' type"""
    return tuple(e.sum() for _, _, _, e, _ in terms)


# ---------------------------------------------------------------------------
# the tables and the states of the GPU tests
# ---------------------------------------------------------------------------
_T = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)
B0 = 0.153
CHAIN = np.zeros((8, 3))
CHAIN[1], CHAIN[3], CHAIN[6], CHAIN[7] = B0 * _T[0], B0 * _T[1], B0 * _T[2], B0 * _T[3]
CHAIN[0] = CHAIN[1] - B0 * _T[2]
CHAIN[4] = CHAIN[3] - B0 * _T[0]
CHAIN[5] = CHAIN[4] + B0 * _T[3]
CHAIN_BONDS = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (2, 6), (2, 7)]
CHAIN_ANGLES = [(0, 1, 2), (1, 2, 3), (1, 2, 6), (1, 2, 7), (3, 2, 6), (3, 2, 7), (6, 2, 7), (2, 3, 4), (3, 4, 5)]
# (atoms, n, phase): three periodicities stacked on 0-1-2-3, every n of 1, 2, 3, 6, phases of both signs
CHAIN_TORSIONS = [((0, 1, 2, 3), 1, 0.0), ((0, 1, 2, 3), 2, np.pi), ((0, 1, 2, 3), 3, 0.4), ((0, 1, 2, 6), 3, 0.0), ((0, 1, 2, 7), 6, -1.1),
                  ((1, 2, 3, 4), 3, 0.0), ((6, 2, 3, 4), 2, 2.5), ((7, 2, 3, 4), 1, -0.7), ((2, 3, 4, 5), 3, np.pi), ((5, 4, 3, 2), 6, 0.9)]
CHAIN_DRUDES = (1, 3, 6)
CHAIN_SLOT = {0: 0, 1: 1, 2: 3, 3: 4, 4: 6, 5: 7, 6: 8, 7: 10}             # atom -> slot within the chain's 11; a Drude right behind its parent
WATER = np.array([[0.0, 0.0, 0.0], [0.09572, 0.0, 0.0], [0.09572 * np.cos(1.82421813), 0.09572 * np.sin(1.82421813), 0.0]])
COLLINEAR = np.array([[1.5, -0.75, 0.25], [1.5625, -0.71875, 0.1875], [1.46875, -0.765625, 0.28125]])     # centre first: a = d, b = -d / 2, dyadic


def bonded_system():
    """-> (DrudeSystem with positions, velocities and the DrudeForce attached, tables = (bonds, angles, torsions) as tables() gives
    them, info: dict of the named rows and slots)"""
    if "system" in _cache:
        return _cache["system"]
    rng = np.random.default_rng(20251020)
    mass, pos, resid, drude_rows = [], [], [], []
    bonds, angles, torsions = [], [], []
    kinds = ["chain"] * CHAINS + ["water"] * WATERS + ["ion"] * (IONS - 2)
    order = rng.permutation(len(kinds))
    kinds = ["ion"] + [kinds[o] for o in order] + ["ion"]           # the far bond's two ions: the first slot and the last
    cells = rng.permutation(6 * 6 * 6)[:len(kinds)]
    centre = lambda c: (np.array([c // 36, (c // 6) % 6, c % 6]) - 2.5) * 0.8                     # noqa: E731
    ions, mol_first = [], []
    n = 0
    for mol, (c, which) in enumerate(zip(cells, kinds)):
        rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]
        mol_first.append(n)
        if which == "chain":
            g = CHAIN @ rot.T + centre(c)
            slot = {a: n + s for a, s in CHAIN_SLOT.items()}
            for a in range(8):
                pos.append(g[a]); mass.append(12.011 - (0.4 if a in CHAIN_DRUDES else 0.0))
                if a in CHAIN_DRUDES:
                    d = rng.normal(size=3)
                    pos.append(g[a] + d / np.linalg.norm(d) * rng.uniform(0.004, 0.01)); mass.append(0.4)
                    drude_rows.append((slot[a] + 1, slot[a], -1, -1, -1, -rng.uniform(1.0, 1.6), rng.uniform(0.0009, 0.0014)))
            for i, j in CHAIN_BONDS:
                bonds.append((slot[i], slot[j], B0 + rng.uniform(-0.004, 0.004), rng.uniform(1.8e5, 2.8e5)))
            for i, j, k in CHAIN_ANGLES:
                angles.append((slot[i], slot[j], slot[k], 1.9106 + rng.uniform(-0.1, 0.1), rng.uniform(300.0, 600.0)))
            for at, per, phase in CHAIN_TORSIONS:
                torsions.append(tuple(slot[a] for a in at) + (per, phase, rng.uniform(0.5, 8.0)))
            resid += [mol] * 11; n += 11
        elif which == "water":
            g = WATER @ rot.T + centre(c)
            pos += list(g); mass += [15.9994, 1.008, 1.008]
            bonds += [(n, n + 1, 0.09572, 4.5e5), (n + 2, n, 0.09572, 4.5e5)]                 # (the second one named H first)
            angles.append((n + 1, n, n + 2, 1.82421813, 460.0))
            resid += [mol] * 3; n += 3
        else:
            pos.append(centre(c)); mass.append(22.99); resid.append(mol); ions.append(n); n += 1
    pos = np.array(pos)
    far_a, far_b = ions[0], ions[-1]
    pair_a, pair_b, zero_a, zero_b = ions[1:5]
    zero_angle, collinear, lone = ions[5:8], ions[8:11], ions[11:-1]
    pos[pair_b] = pos[pair_a] + np.array([0.21, -0.08, 0.12])
    pos[zero_b] = pos[zero_a] + np.array([-0.1, 0.2, 0.05])
    pos[zero_angle[1]], pos[zero_angle[2]] = pos[zero_angle[0]] + np.array([0.15, 0.0, 0.05]), pos[zero_angle[0]] + np.array([-0.02, 0.17, 0.0])
    pos[collinear] = COLLINEAR
    fixed = list(collinear)                                      # no state moves these: their coordinates stay exact in every stored type
    info = dict(far=len(bonds), pair=len(bonds) + 1, zero_bond=len(bonds) + 2, zero_angle=len(angles), collinear=len(angles) + 1,
                far_slots=(far_a, far_b), pair_slots=(pair_a, pair_b), zero_bond_slots=(zero_a, zero_b), zero_angle_slots=tuple(zero_angle),
                collinear_slots=tuple(collinear), lone=tuple(lone), fixed=tuple(fixed), mol_first=np.array(mol_first), busy=None)
    bonds += [(far_a, far_b, float(np.linalg.norm(pos[far_b] - pos[far_a])) - 0.01, 900.0), (pair_a, pair_b, 0.25, 3.0e4),
              (zero_a, zero_b, 0.2, 0.0)]
    angles += [(zero_angle[1], zero_angle[0], zero_angle[2], 1.2, 0.0), (collinear[1], collinear[0], collinear[2], np.pi, 520.0)]
    # the rows of all three tables shuffled; info's row numbers follow
    for key_list, rows in ((("far", "pair", "zero_bond"), bonds), (("zero_angle", "collinear"), angles), ((), torsions)):
        shuffle = rng.permutation(len(rows))
        new_of = np.argsort(shuffle)
        rows[:] = [rows[o] for o in shuffle]
        for key in key_list:
            info[key] = int(new_of[info[key]])
    bf, af, tf = HarmonicBondForce(), HarmonicAngleForce(), PeriodicTorsionForce()
    for r in bonds:
        bf.addBond(*r)
    for r in angles:
        af.addAngle(*r)
    for r in torsions:
        tf.addTorsion(*r)
    tables = (bf.tables(), af.tables(), tf.tables())
    shuffle = rng.permutation(len(drude_rows))                   # row k is pair k: the pairs in an order that is not the slots'
    drude_rows = [drude_rows[o] for o in shuffle]
    df = DrudeForce()
    for r in drude_rows:
        df.addParticle(*r)
    parent_row = {r[1]: k for k, r in enumerate(drude_rows)}
    for first, which in zip(mol_first, kinds):                   # a screened pair inside every chain: the rows of atoms 1 and 3
        if which == "chain":
            df.addScreenedPair(parent_row[first + CHAIN_SLOT[1]], parent_row[first + CHAIN_SLOT[3]], 1.3)
    dt = df.tables()
    mass = np.array(mass)
    vel = rng.normal(size=pos.shape) * np.sqrt(0.0083144626 * 300.0 / mass)[:, None]
    vel[dt[0][:, 0]] = vel[dt[0][:, 1]] + rng.normal(size=(len(dt[0]), 3)) * np.sqrt(0.0083144626 * 1.0 / 0.4)
    s = DrudeSystem(mass=mass, pair_drude=dt[0][:, 0].copy(), pair_parent=dt[0][:, 1].copy(), resid=np.array(resid, np.int32), positions=pos,
                    velocities=vel, name=f"{CHAINS} chains, {WATERS} waters, {IONS} ions")
    s.set_drude_force(df)
    info["busy"] = CHAIN_SLOT[2]                                 # + a chain's first slot: the atom in 4 bonds, 8 angles, 9 torsions
    info["chain_first"] = np.array([f for f, k in zip(mol_first, kinds) if k == "chain"])
    for t in tables + (dt,):
        for a in t:
            a.setflags(write=False)
    _cache["system"] = (s, tables, info)
    return _cache["system"]


def positions(which):
    """the fp64 positions of a state before they are split into the stored types"""
    key = ("positions", which)
    if key not in _cache:
        s, tables, info = bonded_system()
        x = s.positions.copy()
        if which != "lattice":
            rng = np.random.default_rng({"thermal": 1, "stretched": 2}[which])
            first = np.repeat(info["mol_first"], np.diff(np.append(info["mol_first"], len(x))))
            if which == "stretched":
                x = x[first] + 1.25 * (x - x[first])
            x = x + rng.normal(0.0, 0.004 if which == "thermal" else 0.008, x.shape)
            x[list(info["fixed"])] = s.positions[list(info["fixed"])]
        x.setflags(write=False)
        _cache[key] = x
    return _cache[key]


def state(precision, which="lattice"):
    """The stored arrays of a state in a precision and their fp64 reading -> dict: posq [N, 3] (float32 / float64), corr [N, 3]
    float32 or None, x: the positions as the device reads them (fp64).  Built once; callers copy what they change."""
    key = ("state", precision, which)
    if key not in _cache:
        x = positions(which)
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


def results(precision, which, dtype):
    """evaluate() on a state, computed once per (precision, state, type)"""
    key = ("results", precision, which, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = evaluate(bonded_system()[1], state(precision, which)["x"], dtype)
    return _cache[key]


def integrator():
    return DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.0005, 20, 1, True, True)


def receivers(tables):
    return np.unique(np.concatenate([tables[0][0].ravel(), tables[1][0].ravel(), tables[2][0].ravel()]))


# ---------------------------------------------------------------------------
# the tables are what the GPU tests need them to be
# ---------------------------------------------------------------------------
def test_the_tables_have_the_shapes_the_kernel_can_go_wrong_at():
    s, tables, info = bonded_system()
    (bp, bpar), (ap, apar), (tp, tn, tpar) = tables
    n = s.num_particles
    assert n == 722 and n % 32 != 0 and s.num_pairs == 3 * CHAINS
    assert (len(bp), len(ap), len(tp)) == (7 * CHAINS + 2 * WATERS + 3, 9 * CHAINS + WATERS + 2, 10 * CHAINS)
    recv = receivers(tables)
    assert 2 * BLOCK < len(recv) < n and len(recv) % BLOCK != 0                                # three work-groups, the last one ragged
    assert not np.isin(s.pair_drude, recv).any() and not np.isin(info["lone"], recv).any() and len(info["lone"]) >= 10
    for p in (bp, ap, tp):
        assert np.any(np.diff(p[:, 0]) < 0)                                                    # rows not in slot order
    busy = info["chain_first"] + info["busy"]
    for b in busy:
        assert (bp == b).sum() >= 4 and (ap == b).sum() >= 6 and (tp == b).sum() >= 9
    stacked = [tuple(r) for r in tp.tolist()]
    twice = [r for r in set(stacked) if stacked.count(r) >= 2]
    assert twice and all(len({int(tn[k]) for k in range(len(tp)) if tuple(tp[k]) == r}) >= 2 for r in twice)
    assert set(tn.tolist()) == {1, 2, 3, 6} and np.any(tpar[:, 0] > 0) and np.any(tpar[:, 0] < 0) and np.any(tpar[:, 0] == 0)
    assert np.count_nonzero(bpar[:, 1] == 0) == 1 and bpar[info["zero_bond"], 1] == 0
    assert np.count_nonzero(apar[:, 1] == 0) == 1 and apar[info["zero_angle"], 1] == 0
    assert abs(int(bp[info["far"], 0]) - int(bp[info["far"], 1])) > BLOCK
    assert apar[info["collinear"], 0] == np.pi and apar[info["collinear"], 1] > 0
    bond_only = np.setdiff1d(np.unique(bp), np.union1d(np.unique(ap), np.unique(tp)))
    assert set(bond_only) == set(info["far_slots"] + info["pair_slots"] + info["zero_bond_slots"])
    for precision in PRECISIONS:
        for which in STATES:
            st = state(precision, which)
            x = st["x"]
            assert np.array_equal(x[list(info["collinear_slots"])], COLLINEAR)                  # exact in every stored type
            _, _, _, theta = angle_terms(x[ap[:, 0]], x[ap[:, 1]], x[ap[:, 2]], *_columns(apar, np.float64))
            assert theta[info["collinear"]] == np.pi
            others = np.delete(theta, info["collinear"])
            assert np.radians(50) <= others.min() and others.max() <= np.radians(170), (precision, which, np.degrees(others.min()), np.degrees(others.max()))
            for i, j, k in ((0, 1, 2), (1, 2, 3)):                                             # the bond angles inside the torsions
                a, b = x[tp[:, i]] - x[tp[:, j]], x[tp[:, k]] - x[tp[:, j]]
                sin = np.linalg.norm(np.cross(a, b), axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
                assert sin.min() >= 0.3, (precision, which, sin.min())
            if precision == "mixed":
                assert np.count_nonzero(st["corr"]) > 0.8 * st["corr"].size
    r = np.linalg.norm(positions("stretched")[bp[:, 1]] - positions("stretched")[bp[:, 0]], axis=1)
    assert np.median(r / bpar[:, 0]) > 1.15                                                    # far from equilibrium


# ---------------------------------------------------------------------------
# the reference checked against itself, the twin against numpy, the margin
# ---------------------------------------------------------------------------
def _term_inputs(kind, tables, x, dtype):
    """-> (function of the positions alone, positions per role) of one kind of term"""
    (bp, bpar), (ap, apar), (tp, tn, tpar) = tables
    if kind == "bond":
        cols = _columns(bpar, dtype)
        return (lambda xs: bond_terms(*xs, *cols)[:2]), [x[bp[:, m]] for m in range(2)]
    if kind == "angle":
        cols = _columns(apar, dtype)
        return (lambda xs: angle_terms(*xs, *cols)[:2]), [x[ap[:, m]] for m in range(3)]
    cos0, sin0, k = np.cos(tpar[:, 0]).astype(dtype)[:, None], np.sin(tpar[:, 0]).astype(dtype)[:, None], tpar[:, 1].astype(dtype)[:, None]
    return (lambda xs: torsion_terms(*xs, tn, cos0, sin0, k)[:2]), [x[tp[:, m]] for m in range(4)]


@pytest.mark.parametrize("which", STATES)
@pytest.mark.parametrize("kind", KINDS)
def test_forces_against_finite_differences_of_the_energy(kind, which):
    """Every share of every term against -dE/dx by central differences in fp80, h = 1e-6 nm, relative to the term's uncancelled
    scale.  Truncation is h^2 / 6 x the third derivative, which is the share over the square of the shortest length the term
    divides by -- 0.09 nm x sin 0.3 --: 1e-12 / 6 / 7e-4 = 2e-10 of the scale.  Rounding: 2^-64 x E / 2 h with E up to 100 x the
    scale x 1 nm: 3e-12 of it.  Asked for: 1e-8.  The terms with k = 0: exactly 0 on both sides."""
    s, tables, info = bonded_system()
    fn, xs = _term_inputs(kind, tables, state("double", which)["x"].astype(L), L)
    shares, _ = fn(xs)
    scale = [t for t in results("double", which, L) if t[0] == kind][0][4]
    h = L(1e-6)
    worst = np.zeros(len(scale), L)
    for role in range(len(xs)):
        for c in range(3):
            up, dn = [v.copy() for v in xs], [v.copy() for v in xs]
            up[role][:, c] += h; dn[role][:, c] -= h
            worst = np.maximum(worst, np.abs(-(fn(up)[1] - fn(dn)[1]) / (2 * h) - shares[role][:, c]))
    ok = scale > 0
    print(f"{kind} shares against central differences, {which}: {float((worst[ok] / scale[ok]).max()):.2e} of the term's scale, {ok.sum()} terms")
    assert ok.sum() >= len(scale) - 1 and np.all(worst[~ok] == 0)
    assert np.all(worst[ok] <= 1e-8 * scale[ok])
    if kind == "angle":
        assert all(np.all(v[info["collinear"]] == 0) for v in shares)


def test_the_sign_of_the_dihedral_is_the_iupac_one():
    """planar cis: phi = 0; planar trans: phi = pi; and a right-handed twist is positive"""
    for dtype in (np.float64, L):
        x2, x3 = np.array([[0.0, 0.0, 0.0]], dtype), np.array([[0.15, 0.0, 0.0]], dtype)
        x1 = np.array([[-0.05, 0.12, 0.0]], dtype)
        one, zero, k = np.array([[1.0]], dtype), np.array([[0.0]], dtype), np.array([[3.0]], dtype)
        for x4, want in ((np.array([[0.2, 0.12, 0.0]], dtype), (1.0, 0.0)), (np.array([[0.2, -0.12, 0.0]], dtype), (-1.0, 0.0))):
            shares, e, _, (cp, sp) = torsion_terms(x1, x2, x3, x4, np.array([1]), one, zero, k)
            assert (cp[0], sp[0]) == want and e[0] == 3.0 * (1.0 + want[0])                    # E = k (1 + cos phi) at phase 0
            assert all(np.all(np.isfinite(v.astype(np.float64))) for v in shares)
        # looking from p2 to p3 (along +x, y to the left, z up), p4 a quarter turn clockwise from p1: phi = +pi/2
        x4 = np.array([[0.2, 0.0, 0.12]], dtype)
        _, _, _, (cp, sp) = torsion_terms(x1, x2, x3, x4, np.array([1]), one, zero, k)
        assert cp[0] == 0.0 and sp[0] == 1.0


@pytest.mark.parametrize("which", STATES)
def test_every_terms_shares_and_torques_add_up_to_zero(which):
    """In the reference: the shares of a term sum to zero and so do their torques about the origin, within 2^-58 of the term's scale
    (x the largest |coordinate| of its atoms, for the torque): sums of three or four products rounded to 2^-64 each."""
    room = L(2.0) ** -58
    s, tables, info = bonded_system()
    x = state("double", which)["x"].astype(L)
    for kind, slots, shares, _, scale in results("double", which, L):
        force = sum(shares)
        torque = sum(_cross(x[sl], v) for sl, v in zip(slots, shares))
        reach = np.max([np.abs(x[sl]).max(1) for sl in slots], axis=0)
        f, t = np.abs(force).max(1), np.abs(torque).max(1)
        ok = scale > 0
        print(f"{kind}, {which}: shares sum to {float((f[ok] / scale[ok]).max()):.2e} of the scale, torques to {float((t[ok] / (scale[ok] * reach[ok])).max()):.2e} of scale x reach")
        assert np.all(f <= room * scale) and np.all(t <= room * scale * reach)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_twins_bond_shares_are_five_lines_of_numpy(precision):
    s, tables, info = bonded_system()
    bp, bpar = tables[0]
    x = state(precision, "thermal")["x"]
    d = x[bp[:, 1]] - x[bp[:, 0]]
    r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    f = ((bpar[:, 1] * (r - bpar[:, 0])) / r)[:, None] * d
    kind, slots, shares, _, _ = results(precision, "thermal", np.float64)[0]
    assert kind == "bond" and np.array_equal(slots[0], bp[:, 0]) and np.array_equal(slots[1], bp[:, 1])
    assert np.array_equal(shares[0].view(np.uint64), f.view(np.uint64)) and np.array_equal(shares[1].view(np.uint64), (-f).view(np.uint64))
    assert np.all(shares[0][info["zero_bond"]] == 0)


def margins():
    """-> (shares, energies): the largest difference between twin and reference per term over the term's uncancelled scale, and of
    the three energies over the sum of |term energies|, over the states and the stored types"""
    worst, worst_e = {k: 0.0 for k in KINDS}, 0.0
    for precision in PRECISIONS:
        for which in STATES:
            ref, twin = results(precision, which, L), results(precision, which, np.float64)
            for (kind, _, rs, re, scale), (_, _, ts, te, _) in zip(ref, twin):
                d = np.max([np.abs(t.astype(L) - r).max(1) for r, t in zip(rs, ts)], axis=0)
                ok = scale > 0
                assert np.all(d[~ok] == 0)                       # (k = 0: shares of exactly 0 in both)
                worst[kind] = max(worst[kind], float((d[ok] / scale[ok]).max()))
                worst_e = max(worst_e, float(abs(L(te.sum()) - re.sum()) / np.abs(re).sum()))
    return worst, worst_e


def test_the_margin_between_twin_and_reference():
    """MEASURED_MARGIN of the module docstring, measured: it must cover the figure, and not by more than a quarter."""
    figure, energy = margins()
    print(f"fp64 twin against the fp80 reference: shares {figure} of the term's uncancelled scale, energies {energy:.3e} of the sum of "
          f"|term energies|; MEASURED_MARGIN {MEASURED_MARGIN:.2e}, the GPU gate {GATE:.2e}")
    assert 0.75 * MEASURED_MARGIN <= max(figure.values()) <= MEASURED_MARGIN
    assert energy <= MEASURED_MARGIN


def test_rows_with_k_zero_and_the_collinear_angle_contribute_exactly_nothing():
    s, tables, info = bonded_system()
    for dtype in (np.float64, L):
        for which in STATES:
            bond, angle, _ = results("mixed", which, dtype)
            assert bond[3][info["zero_bond"]] == 0 and all(np.all(v[info["zero_bond"]] == 0) for v in bond[2])
            for row in (info["zero_angle"], info["collinear"]):
                assert all(np.all(v[row] == 0) and np.all(np.isfinite(v[row].astype(np.float64))) for v in angle[2])
                # (theta0 is the fp64 pi: against fp80's the reference keeps an energy of 1/2 k (1.2e-16)^2)
                assert angle[3][row] == 0 or (dtype is L and row == info["collinear"] and angle[3][row] < 1e-29)


# ---------------------------------------------------------------------------
# tgnh_set_bonded_forces on a host-only handle
# ---------------------------------------------------------------------------
def host(s):
    return HostTopology(s, integrator())


def counts(top):
    out = (C.c_int * 3)()
    assert top.lib.tgnh_get_num_bonded_terms(top.h, out) == _lib.TGNH_OK
    return tuple(out)


def refused(top, tables, match, status=_lib.ERR_ARG):
    before = counts(top)
    with pytest.raises(TgnhError, match=match) as e:
        BondedForces(top, *tables)
    assert e.value.status == status
    assert counts(top) == before                                                                # refused tables change nothing


def test_accepted_tables_and_the_counts():
    s, tables, info = bonded_system()
    top = host(s)
    assert counts(top) == (0, 0, 0)
    f = BondedForces(top, *tables)
    want = tuple(len(t[0]) for t in tables)
    assert f.num_terms == want == counts(top)
    g = BondedForces(top, bonds=(tables[0][0][:5], tables[0][1][:5]))                           # a second set replaces the first, all three
    assert g.num_terms == (5, 0, 0) == f.num_terms
    BondedForces(top, torsions=tables[2])
    assert counts(top) == (0, 0, want[2])
    dup = (np.concatenate([tables[2][0], tables[2][0][:7]]), np.concatenate([tables[2][1], tables[2][1][:7]]), np.concatenate([tables[2][2], tables[2][2][:7]]))
    BondedForces(top, (np.concatenate([tables[0][0]] * 2), np.concatenate([tables[0][1]] * 2)), tables[1], dup)      # duplicate terms are allowed
    assert counts(top) == (2 * want[0], want[1], want[2] + 7)
    f.clear()
    assert counts(top) == (0, 0, 0)
    BondedForces(top)                                                                           # nothing at all: the empty tables
    assert counts(top) == (0, 0, 0)
    # the launching calls on a host-only handle
    f = BondedForces(top, *tables)
    out = np.zeros(3)
    for call in (f.compute, lambda: f.compute(energy=True), f.energy):
        with pytest.raises(TgnhError, match="host-only") as e:
            call()
        assert e.value.status == _lib.ERR_STATE
    assert top.lib.tgnh_get_bonded_energy(top.h, None, None) == _lib.ERR_ARG
    assert top.lib.tgnh_get_num_bonded_terms(top.h, None) == _lib.ERR_ARG
    assert top.lib.tgnh_get_num_bonded_terms(None, None) == _lib.ERR_ARG
    assert top.lib.tgnh_set_bonded_forces(None, 0, None, None, 0, None, None, 0, None, None, None) == _lib.ERR_ARG
    assert top.lib.tgnh_get_bonded_energy(top.h, None, out.ctypes.data_as(_lib.c_f64p)) == _lib.ERR_STATE
    top.close()


def test_refusals():
    s, tables, info = bonded_system()
    (bp, bpar), (ap, apar), (tp, tn, tpar) = [[a.copy() for a in t] for t in tables]
    n = s.num_particles
    top = host(s)
    lib = top.lib
    i32, f64 = lambda v: v.ctypes.data_as(_lib.c_i32p), lambda v: v.ctypes.data_as(_lib.c_f64p)

    def raw(nb=len(bp), na=len(ap), nt=len(tp), drop=None):
        args = [nb, i32(bp), f64(bpar), na, i32(ap), f64(apar), nt, i32(tp), i32(tn), f64(tpar)]
        if drop is not None:
            args[drop] = None
        return lib.tgnh_set_bonded_forces(top.h, *args)

    def with_(table, array, row, col, value):
        t = [[a.copy() for a in t] for t in ((bp, bpar), (ap, apar), (tp, tn, tpar))]
        if col is None:
            t[table][array][row] = value
        else:
            t[table][array][row, col] = value
        return t
    for trial in (0, 1):                                         # on empty tables, then on tables in force
        before = counts(top)
        for kw in (dict(nb=-1), dict(na=-3), dict(nt=-2 ** 31)):
            assert raw(**kw) == _lib.ERR_ARG and b"negative count" in lib.tgnh_last_error()
        for drop in (1, 2, 4, 5, 7, 8, 9):
            assert raw(drop=drop) == _lib.ERR_ARG and b"null array" in lib.tgnh_last_error()
        # more entries than 32-bit offsets take: decided from the counts, before any row is read
        for kw in (dict(nb=2 ** 30), dict(na=2 ** 30 - 1), dict(nt=2 ** 29), dict(nb=2 ** 29, na=2 ** 28, nt=2 ** 27)):
            assert raw(**kw) == _lib.ERR_UNSUPPORTED and b"32-bit offsets" in lib.tgnh_last_error()
        assert counts(top) == before
        refused(top, with_(0, 0, 5, 1, n), "bond 5: index %d out of range" % n)
        refused(top, with_(0, 0, 0, 0, -1), "bond 0: index -1 out of range")
        refused(top, with_(1, 0, 7, 2, n + 3), "angle 7: index %d out of range" % (n + 3))
        refused(top, with_(2, 0, 11, 3, -2), "torsion 11: index -2 out of range")
        refused(top, with_(0, 0, 4, 1, bp[4, 0]), "bond 4 names particle %d twice" % bp[4, 0])
        refused(top, with_(1, 0, 3, 2, ap[3, 0]), "angle 3 names particle %d twice" % ap[3, 0])
        refused(top, with_(1, 0, 3, 1, ap[3, 2]), "angle 3 names particle %d twice" % ap[3, 2])
        refused(top, with_(2, 0, 9, 3, tp[9, 0]), "torsion 9 names particle %d twice" % tp[9, 0])
        refused(top, with_(2, 0, 9, 2, tp[9, 1]), "torsion 9 names particle %d twice" % tp[9, 1])
        for bad in (np.nan, np.inf, -np.inf):
            refused(top, with_(0, 1, 6, 0, bad), "bond 6: the length is not finite")
            refused(top, with_(0, 1, 6, 1, bad), "bond 6: k is not finite")
            refused(top, with_(1, 1, 2, 0, bad), "angle 2: the angle is not finite")
            refused(top, with_(1, 1, 2, 1, bad), "angle 2: k is not finite")
            refused(top, with_(2, 2, 8, 0, bad), "torsion 8: the phase is not finite")
            refused(top, with_(2, 2, 8, 1, bad), "torsion 8: k is not finite")
        refused(top, with_(0, 1, 1, 0, -1e-9), "bond 1: the length is negative")
        refused(top, with_(1, 1, 1, 0, -1e-9), r"angle 1: the angle is outside \[0, pi\]")
        refused(top, with_(1, 1, 1, 0, np.nextafter(np.pi, 4.0)), r"angle 1: the angle is outside \[0, pi\]")
        for bad in (0, -1):
            refused(top, with_(2, 1, 3, None, bad), "torsion 3: periodicity %d is below 1" % bad)
        refused(top, with_(2, 1, 3, None, 13), "torsion 3: periodicity 13 is above 12", _lib.ERR_UNSUPPORTED)
        # what is legal: a length of 0, the ends of [0, pi], k = 0 and k < 0, periodicity 12, any finite phase
        ok = with_(0, 1, 1, 0, 0.0)
        ok[1][1][1, 0], ok[1][1][2, 0], ok[0][1][3, 1], ok[2][1][3], ok[2][2][5, 0] = 0.0, np.pi, -5.0, 12, 100.0
        BondedForces(top, *ok)
        assert counts(top) == (len(bp), len(ap), len(tp))
    top.close()


# ---------------------------------------------------------------------------
# forces.HarmonicBondForce, HarmonicAngleForce, PeriodicTorsionForce, BondedForces
# ---------------------------------------------------------------------------
def test_the_table_classes_round_trip_their_parameters():
    b = HarmonicBondForce()
    assert b.getNumBonds() == 0 and b.addBond(0, 1, 0.1, 1000.0) == 0 and b.addBond(2, 1, 0.15, 2.5e5) == 1
    assert b.getBondParameters(1) == (2, 1, 0.15, 2.5e5)
    b.setBondParameters(0, 3, 4, 0.2, 0.0)
    assert b.getBondParameters(0) == (3, 4, 0.2, 0.0) and b.getNumBonds() == 2
    a = HarmonicAngleForce()
    assert a.getNumAngles() == 0 and a.addAngle(0, 1, 2, 1.9, 400.0) == 0
    a.setAngleParameters(0, 2, 1, 0, 2.0, 300.0)
    assert a.getAngleParameters(0) == (2, 1, 0, 2.0, 300.0) and a.getNumAngles() == 1
    t = PeriodicTorsionForce()
    assert t.getNumTorsions() == 0 and t.addTorsion(0, 1, 2, 3, 3, 0.0, 1.5) == 0 and t.addTorsion(0, 1, 2, 3, 2, np.pi, 0.5) == 1
    assert t.getTorsionParameters(1) == (0, 1, 2, 3, 2, np.pi, 0.5)
    t.setTorsionParameters(0, 3, 2, 1, 0, 6, -0.5, 2.0)
    assert t.getTorsionParameters(0) == (3, 2, 1, 0, 6, -0.5, 2.0) and t.getNumTorsions() == 2
    for table, get, put, row in ((b, b.getBondParameters, b.setBondParameters, (0, 1, 0.1, 1.0)), (a, a.getAngleParameters, a.setAngleParameters, (0, 1, 2, 1.0, 1.0)),
                                 (t, t.getTorsionParameters, t.setTorsionParameters, (0, 1, 2, 3, 1, 0.0, 1.0))):
        for bad in (-1, len(table.tables()[0])):
            with pytest.raises(IndexError, match="Index out of range"):
                get(bad)
            with pytest.raises(IndexError, match="Index out of range"):
                put(bad, *row)
    p, q = b.tables()
    assert p.dtype == np.int32 and p.tolist() == [[3, 4], [2, 1]] and q.dtype == np.float64 and q.tolist() == [[0.2, 0.0], [0.15, 2.5e5]]
    p, q = a.tables()
    assert p.dtype == np.int32 and p.tolist() == [[2, 1, 0]] and q.dtype == np.float64 and q.tolist() == [[2.0, 300.0]]
    p, per, q = t.tables()
    assert p.dtype == np.int32 and p.tolist() == [[3, 2, 1, 0], [0, 1, 2, 3]] and per.dtype == np.int32 and per.tolist() == [6, 2]
    assert q.dtype == np.float64 and q.tolist() == [[-0.5, 2.0], [np.pi, 0.5]]
    assert [x.shape for x in HarmonicBondForce().tables()] == [(0, 2), (0, 2)]
    assert [x.shape for x in HarmonicAngleForce().tables()] == [(0, 3), (0, 2)]
    assert [x.shape for x in PeriodicTorsionForce().tables()] == [(0, 4), (0,), (0, 2)]


class _Recorder:
    """stands where the library stands and writes down every call"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return _lib.TGNH_OK
        return fn


class _Owner:
    def __init__(self):
        self.lib, self.h = _Recorder(), C.c_void_p(1)

    def _stream(self):
        return None


def test_shape_refusals_make_no_library_call():
    s, tables, info = bonded_system()
    (bp, bpar), (ap, apar), (tp, tn, tpar) = tables
    bad = [dict(bonds=(bp, bpar[:5])), dict(bonds=(bp[:, :1], bpar)), dict(bonds=(ap, apar)), dict(bonds=(bp, bpar, bpar)), dict(bonds=(bp.ravel(), bpar)),
           dict(angles=(ap[:3], apar)), dict(angles=(bp, bpar)), dict(angles=(ap, apar[:, :1])),
           dict(torsions=(tp, tn[:4], tpar)), dict(torsions=(tp, tpar)), dict(torsions=(tp[:9], tn, tpar)), dict(torsions=(tp, tn, tpar[:2])),
           dict(torsions=(ap, tn, tpar)), dict(bonds=tables[0], angles=tables[1], torsions=(tp, tn[:, None], tpar))]
    for kw in bad:
        owner = _Owner()
        with pytest.raises(TgnhError, match="set_bonded_forces: ") as e:
            BondedForces(owner, **kw)
        assert e.value.status == _lib.ERR_ARG and owner.lib.calls == [], kw
    owner = _Owner()                                             # and what fits makes exactly one
    f = BondedForces(owner, tables[0], None, tables[2])
    assert [c[0] for c in owner.lib.calls] == ["tgnh_set_bonded_forces"]
    args = owner.lib.calls[0][1]
    assert (args[1], args[4], args[7]) == (len(bp), 0, len(tp)) and args[5] is None and args[6] is None
    f.clear()
    assert owner.lib.calls[1] == ("tgnh_set_bonded_forces", (owner.h, 0, None, None, 0, None, None, 0, None, None, None))
    seen = []
    owner.force = type("F", (), {"zero_": lambda self: seen.append("zero"), "data_ptr": lambda self: 64})()
    both = f.then(lambda ctx: seen.append("then"))
    both(owner)
    assert seen == ["zero", "then"] and owner.lib.calls[2] == ("tgnh_compute_bonded_forces", (owner.h, 64, 0, None))
