"""Shared helpers for the parity tests (oracle = checker, HIP library = thing under test)."""
import numpy as np

from openmm_drudenose_amd import synth
from oracle import Oracle, MODE_DUALNH, MODE_TGNH

ONE_4PI_EPS0 = 138.935456          # OpenMM SimTKOpenMMRealType.h
MODES = {"dualNH": MODE_DUALNH, "TGNH": MODE_TGNH}


def rel_err(a, b):
    """max-norm relative error: max|a-b| / max|b|."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / (den if den > 0 else 1.0))


def make_oracle(system, group, ngroups, mode, integ):
    return Oracle.from_integrator(system, integ, group, ngroups, MODES[mode])


def oracle_run(o, system, nsteps, k_drude=synth.K_DRUDE, k_tether=synth.K_TETHER, record=False, x0=None):
    """Runs the oracle with the harness force; returns final (pos, vel) and optionally per-step KE/scale.
    x0 = tether sites; pass ctx.sites() so the oracle sees the sites exactly as the HIP harness stores them."""
    pos, vel = system.positions.copy(), system.velocities.copy()
    x0 = system.positions.copy() if x0 is None else np.ascontiguousarray(x0, np.float64)
    f = o.harness_force(pos, x0, k_drude, k_tether)
    if not record:
        o.run_harness(pos, vel, f, x0, k_drude, k_tether, nsteps)
        return pos, vel
    kes, scs = [], []
    for _ in range(nsteps):
        ke, sc = o.propagate_nhc(vel)
        kes.append(ke); scs.append(sc)
        o.half_kick(vel, f)
        o.drift(pos, vel)
        o.hardwall(pos, vel)
        f = o.harness_force(pos, x0, k_drude, k_tether)
        o.half_kick(vel, f)
        ke, sc = o.propagate_nhc(vel)
        kes.append(ke); scs.append(sc)
    return pos, vel, np.array(kes), np.array(scs)


def to_internal(x, mode):
    """Oracle thermostat vectors -> the library's NT layout (dualNH: [real, 0, drude])."""
    x = np.asarray(x)
    if mode == "dualNH":
        return np.array([x[0], 0.0, x[1]]) if x.ndim == 1 else np.stack([x[:, 0], 0 * x[:, 0], x[:, 1]], 1)
    return x


def extended_energy(system, normal, pos, vel, x0, nkt, eta, eta_dot, eta_mass, chains, kT, kT_drude, mode,
                    k_drude=synth.K_DRUDE, k_tether=synth.K_TETHER):
    """The quantity Nose-Hoover-chain dynamics conserves, for the harness force field:
        H = 1/2 sum m v^2 + U + sum_t [ sum_i 1/2 Q_ti etaDot_ti^2 + NkT_t eta_t0 + kT_t sum_{i>=1} eta_ti ].
    The reference never evaluates it (it is the invariant SURVEY 8c(3) asks the build to add); a restatement whose
    chain, KE partition or rescale were wrong in sign, factor or coupling would drift linearly instead of
    fluctuating at O(dt^2).  Thermostat arrays: TGNH [thermostat][link] (etaDot rows of C+1); dualNH the reference's
    interleaved [real0, drude0, real1, drude1, ...] (Ref :186-217), valid with useDrudeNHChains only."""
    m = system.mass
    ke = 0.5 * float((m[:, None] * vel ** 2).sum())
    tether = np.zeros(len(m), bool)
    tether[normal] = True
    tether[system.pair_parent] = True
    tether &= m > 0
    sep = pos[system.pair_drude] - pos[system.pair_parent]
    pe = 0.5 * k_tether * float(((pos - x0)[tether] ** 2).sum()) + 0.5 * k_drude * float((sep ** 2).sum())
    C = chains
    if mode == "dualNH":
        eta, eta_dot, eta_mass = (np.asarray(a)[:2 * C].reshape(C, 2).T for a in (eta, eta_dot, eta_mass))
    else:
        nt = len(nkt)
        eta, eta_dot, eta_mass = (np.asarray(a).reshape(nt, -1)[:, :C] for a in (eta, eta_dot, eta_mass))
    th = 0.0
    for t in range(len(nkt)):
        if eta_mass[t, 0] <= 0:                       # inert thermostat (Cu :561 etaMass > 0 guard)
            continue
        kt = kT_drude if t == len(nkt) - 1 else kT
        th += 0.5 * float((eta_mass[t] * eta_dot[t] ** 2).sum()) + nkt[t] * eta[t, 0] + kt * float(eta[t, 1:].sum())
    return ke + pe + th, ke, th


def random_topology(seed):
    """Ragged test input: molecules of 1-40 slots (every third seed: two longer than a tile), Drude pairs anywhere inside
    a molecule (Drude before or after its parent, up to 30 slots apart), massless sites, 1-6 temperature groups assigned
    per molecule, a few constraints inside molecules."""
    rng = np.random.default_rng(1000 + seed)
    sizes = rng.integers(1, 41, size=rng.integers(40, 400))
    if seed % 3 == 0:
        sizes[rng.integers(0, len(sizes), 2)] = rng.integers(600, 1500, 2)
    n = int(sizes.sum())
    resid = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    first = np.r_[0, np.cumsum(sizes)[:-1]]
    mass = rng.uniform(1.0, 40.0, n)
    ngroups = int(rng.integers(1, 7))
    group = np.repeat(rng.integers(0, ngroups, len(sizes)), sizes).astype(np.int32)
    pd, pp, used = [], [], np.zeros(n, bool)
    for f, sz in zip(first, sizes):
        for _ in range(int(rng.integers(0, max(1, sz // 2) + 1))):
            a = f + int(rng.integers(0, sz))
            b = a + int(rng.integers(-30, 31))
            if b == a or b < f or b >= f + sz or used[a] or used[b]:
                continue
            used[a] = used[b] = True
            pd.append(a); pp.append(b)
            mass[a] = 0.4
    free = np.flatnonzero(~used)
    mass[rng.choice(free, size=min(len(free), n // 20), replace=False)] = 0.0
    for f, sz in zip(first, sizes):                      # every molecule keeps a massive particle (else v_com is 0/0: rejected)
        if not mass[f:f + sz].any():
            mass[f] = 12.0
    cons = []
    for f, sz in zip(first, sizes):
        if sz >= 3 and rng.random() < 0.3:
            i, j = f + rng.choice(sz, 2, replace=False)
            if mass[i] > 0 and mass[j] > 0:
                cons.append((i, j))
    return mass, pd, pp, resid, group, ngroups, cons, sizes, first, rng


def random_clusters(rng, mass, pd, pp, sizes, first, pos):
    """Constraint clusters for a random_topology: in about half of the molecules, 2-4 massive atoms outside Drude pairs are
    pulled to within ~0.1 nm of one another and held at those distances -- all pairs (a rigid body, up to 3 atoms) or the bonds from
    the first atom only.  -> (cluster_atoms [K,4], cluster_dist [K,6]) in DrudeSystem's canonical pair order."""
    PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
    in_pair = np.zeros(len(mass), bool)
    in_pair[pd] = True
    in_pair[pp] = True
    atoms, dist = [], []
    for f, sz in zip(first, sizes):
        cand = [i for i in range(f, f + sz) if mass[i] > 0 and not in_pair[i]]
        if len(cand) < 2 or rng.random() < 0.5:
            continue
        c = int(rng.integers(2, min(4, len(cand)) + 1))
        pick = rng.choice(cand, c, replace=False)
        for k in range(1, c):
            pos[pick[k]] = pos[pick[0]] + rng.normal(0.0, 0.06, 3) + np.array([0.08, 0.0, 0.0])
        rigid = c <= 3 and rng.random() < 0.5            # (a random rigid tetrahedron can take SHAKE > 500 sweeps at 1e-10)
        a = [-1] * 4
        a[:c] = [int(x) for x in pick]
        d = [0.0] * 6
        for k, (i, j) in enumerate(PAIRS):
            if j < c and (rigid or i == 0):
                d[k] = float(np.linalg.norm(pos[pick[i]] - pos[pick[j]]))
        atoms.append(a)
        dist.append(d)
    return np.array(atoms, np.int32).reshape(-1, 4), np.array(dist, np.float64).reshape(-1, 6)


# ---- water boxes with more than one wave pattern (tests/test_host_logic.py, tests/test_velocity_planes_gpu.py) ----
def water_variants(n, group_of=None, heavy_of=None):
    """synth.water_box(n) with temperature groups dealt per molecule and some molecules' hydrogens made heavy: group_of and heavy_of
    take the array of molecule indices 0 .. n - 1 and return a group (0 .. G - 1, every one of them used) resp. a truth value per
    molecule; the two H masses are 2.0 where heavy_of holds, set before the velocities are drawn (they are thermal for the masses
    the box really has).  With neither it IS synth.water_box(n): same seed, same draws.  -> (DrudeSystem, group[N], G)"""
    rng = np.random.default_rng(synth.SEED)
    mass, pd, pp, resid, pos = synth._molecules(n, synth._W_TEST, 0.31)
    m = np.arange(n)
    g = np.zeros(n, np.int64) if group_of is None else np.asarray(group_of(m), np.int64)
    ng = int(g.max()) + 1
    assert g.shape == (n,) and g.min() >= 0 and len(np.unique(g)) == ng
    if heavy_of is not None:
        heavy = np.asarray(heavy_of(m), bool)
        mass.reshape(n, 5)[heavy, 2:4] = 2.0               # slots 2, 3: H1, H2 (synth._W_TEST)
    out = synth._finish(mass, pd, pp, resid, pos, np.repeat(g, 5).astype(np.int32), ng, rng, 300.0, 1.0, f"swm4-{n}-variant")
    out[0].lattice = (5, int(np.ceil(n ** (1.0 / 3.0) - 1e-9)), 0.31, np.asarray(synth._W_TEST["geom"], np.float64), 0)   # (synth.water_box)
    return out


# The rows of the wave-pattern table: name -> (group_of, heavy_of, what the row is).  A wave tile of these boxes
# holds 12 molecules = 60 slots; the groups of `mod k` repeat after k molecules = 5 k slots.
def _mod(k):
    return lambda m: m % k


WATER_ROWS = {
    "mod2": (_mod(2), None), "mod3": (_mod(3), None), "mod4": (_mod(4), None), "mod5": (_mod(5), None), "mod6": (_mod(6), None),
    "mod8": (_mod(8), None),
    "group-per-tile": (lambda m: (m // 12) % 4, None),
    "group-per-tile3": (lambda m: (m // 12) % 3, None),
    "heavy-tiles": (None, lambda m: (m // 12) % 2 == 1),           # equal words, other masses: a pattern id of their own
    "heavy-every-third-tile": (None, lambda m: (m // 12) % 3 == 1),
    "heavy-odd": (None, lambda m: m % 2 == 1),                     # the words repeat after 5 slots, the masses after 10
    "plain": (None, None),
}
_WATER_VARIANTS = {}


def water_row(name, n):
    """water_variants of a row of WATER_ROWS, built once per (row, n) and shared: nobody writes to what this returns"""
    if (name, n) not in _WATER_VARIANTS:
        _WATER_VARIANTS[name, n] = water_variants(n, *WATER_ROWS[name])
    return _WATER_VARIANTS[name, n]


# ---- topologies the tiled kernels cannot hold: they step on the gather path (tgnh_gather.hip; tests/test_gather_gpu.py) ----
def drudes_at_the_end(n_mol, seed=3):
    """A water box as some builders write it: all atoms first (O, H, H, M per molecule), all Drude particles appended behind them.
    Every Drude is far from its parent, and every residue comes in two runs."""
    s, _, _ = synth.water_box(n_mol)
    d = np.asarray(s.pair_drude)
    keep = np.setdiff1d(np.arange(s.num_particles), d)
    order = np.r_[keep, d]                                    # new -> old
    inv = np.empty_like(order); inv[order] = np.arange(len(order))
    out = synth.DrudeSystem(mass=s.mass[order], pair_drude=inv[s.pair_drude].astype(np.int32), pair_parent=inv[s.pair_parent].astype(np.int32),
                            resid=s.resid[order], positions=s.positions[order], velocities=s.velocities[order], name="drudes-at-the-end")
    return out, np.zeros(out.num_particles, np.int32), 1


def onion(n=700, seed=5):
    """One molecule whose pairs nest like onion skins (i, n - 1 - i): every cut between slot 1 and n - 1 goes through a pair."""
    rng = np.random.default_rng(seed)
    mass = rng.uniform(8.0, 20.0, n)
    pd, pp = np.arange(n // 2, dtype=np.int32), (n - 1 - np.arange(n // 2)).astype(np.int32)
    mass[pd] = 0.4
    pos = rng.uniform(0.0, 2.0, (n, 3))
    pos[pd] = pos[pp] + rng.normal(0.0, 0.002, (n // 2, 3))
    return synth._finish(mass, pd, pp, np.zeros(n, np.int32), pos, np.zeros(n, np.int32), 1, rng, 300.0, 1.0, "onion")


def far_pairs(seed=7):
    """Water-like molecules plus one 1400-slot molecule whose Drude particles sit 600-1200 slots from their parents."""
    rng = np.random.default_rng(seed)
    s, g, ng = synth.mixed(200, 10)
    n0, nb = s.num_particles, 1400
    mass = np.r_[s.mass, rng.uniform(6.0, 30.0, nb)]
    parents = n0 + np.arange(0, 100)
    drudes = n0 + nb - 1 - np.arange(0, 100) * 2
    mass[drudes] = 0.4
    resid = np.r_[s.resid, np.full(nb, s.resid.max() + 1)].astype(np.int32)
    group = np.r_[g, np.full(nb, 1)].astype(np.int32)
    pos = np.r_[s.positions, rng.uniform(0.0, 4.0, (nb, 3))]
    pos[drudes] = pos[parents] + rng.normal(0.0, 0.002, (100, 3))
    out = synth._finish(mass, np.r_[s.pair_drude, drudes].astype(np.int32), np.r_[s.pair_parent, parents].astype(np.int32), resid, pos,
                        group, ng, rng, 300.0, 1.0, "far-pairs")
    return out


def scattered_residues(seed=11):
    """The mixed box with its residue array in random order: every residue comes in many runs, and the reference's walk of `count`
    particles from a residue's last run (K :90-91) leaves the array for the residues whose last run lies near its end.  One
    temperature group (a Drude particle and its parent must share theirs, Ref :128-131, and the shuffle parts them from any other)."""
    s, g, _ = synth.mixed(120, 10)
    resid = s.resid.copy()
    np.random.default_rng(seed).shuffle(resid)
    out = synth.DrudeSystem(mass=s.mass, pair_drude=s.pair_drude, pair_parent=s.pair_parent, resid=resid, positions=s.positions,
                            velocities=s.velocities, name="scattered-residues")
    return out, np.zeros_like(g), 1


def far_pairs_at_size(n_water=400_000, long=((10_000, 1_000), (40_000, 10_000), (100_000, 50_000)), seed=9):
    """far_pairs at size: `n_water` water-like molecules and ions (the mixed box, four groups), then long contiguous molecules of
    (slots, distance): in every block of 2 x distance slots, the Drude particles of the block's first half sit `distance` slots
    behind their parents in its second half (every other slot of it).  The COM is a molecule's own here (every residue one run),
    and the longest residue is walked by one team of gather_com_kernel."""
    rng = np.random.default_rng(seed)
    s, g, ng = synth.mixed(n_water, 1000)
    mass, resid, group, pos = [s.mass], [s.resid], [g], [s.positions]
    pd, pp = [s.pair_drude], [s.pair_parent]
    start, r = s.num_particles, int(s.resid.max()) + 1
    for size, dist in long:
        assert size % (2 * dist) == 0
        m = rng.uniform(6.0, 30.0, size)
        blocks = start + np.arange(0, size, 2 * dist)[:, None]
        par = (blocks + np.arange(0, dist, 2)[None, :]).ravel()
        m[par + dist - start] = 0.4
        pp.append(par); pd.append(par + dist)
        mass.append(m); resid.append(np.full(size, r)); group.append(np.full(size, 1))
        pos.append(rng.uniform(0.0, 20.0, (size, 3)))
        start += size
        r += 1
    return synth._finish(np.concatenate(mass), np.concatenate(pd).astype(np.int32), np.concatenate(pp).astype(np.int32),
                         np.concatenate(resid).astype(np.int32), np.concatenate(pos), np.concatenate(group).astype(np.int32), ng, rng,
                         300.0, 1.0, "far-pairs-at-size")


def interleaved(n_mol=60):
    """Two particles of neighbouring molecules swapped: residues 0 and 1 each come in several runs.  The reference's table says
    (count, start of the LAST run) for them (Cu :121-124) and its COM kernel walks `count` particles from there (K :90-91),
    whoever they belong to -- reproduced as it is, here and in the oracle (well inside the array for these two)."""
    s, g, ng = synth.water_box(n_mol)
    resid = s.resid.copy()
    resid[[1, 6]] = resid[[6, 1]]
    out = synth.DrudeSystem(mass=s.mass, pair_drude=s.pair_drude, pair_parent=s.pair_parent, resid=resid, positions=s.positions,
                            velocities=s.velocities, name="interleaved")
    return out, g, ng


# ---- the hard wall's taken branch (tests/test_hardwall.py, tests/test_hardwall_gpu.py) ----
WALL_MUTANTS = ("swap_masses_in_vbond", "no_clamp", "bond_dir_reversed", "parent_not_updated", "wrong_temperature", "no_wall")


def hardwall_reference(pos, vel, mass, pair_drude, pair_parent, max_dist, dt, kT_drude, mutant=None):
    """The reference's hard wall (Ref :298-363 ; Cu :471-574) in np.longdouble, in its own two-member form (p1 = Drude, p2 =
    parent), every pair at once (pairs share no particle, so their order does not matter).  Independent of the oracle and of the
    kernels' self / partner formulation.  No throw beyond twice the wall (K has none): `ratio` says where that happened.
    -> (pos, vel) as float64 and the decision quantities per pair:
        ratio   r / max_dist before the wall          out     ratio > 1: the pair bounced
        dt_raw  the unclamped deltaR / |dotvr1 - dotvr2| over dt (inf where the speeds are equal)
        dotvr1, dotvr2   the centred radial speeds (of a massless parent: the Drude's own, and 0)
        vperp   |vp1 - vp2|, the relative speed across the bond, which the wall must leave alone
    mutant: one of WALL_MUTANTS, a deliberate mis-restatement (what the sensitivity tests compare the true one with)."""
    L = np.longdouble
    assert mutant is None or mutant in WALL_MUTANTS
    pos, vel = np.array(pos, L), np.array(vel, L)
    p1, p2 = np.asarray(pair_drude), np.asarray(pair_parent)
    mass1, mass2 = np.asarray(mass, L)[p1], np.asarray(mass, L)[p2]
    max_dist, dt = L(max_dist), L(dt)
    hws = np.sqrt(L(kT_drude) * (25 if mutant == "wrong_temperature" else 1))          # Ref :300
    delta = pos[p1] - pos[p2]
    if mutant == "bond_dir_reversed":
        delta = -delta
    r = np.sqrt((delta * delta).sum(1))
    rInv = 1 / r
    out = rInv * max_dist < 1                                                        # Ref :307
    bondDir = delta * rInv[:, None]
    vel1, vel2 = vel[p1], vel[p2]
    deltaR = r - max_dist
    dotvr1 = (vel1 * bondDir).sum(1)
    vp1 = vel1 - bondDir * dotvr1[:, None]
    massless = mass2 == 0
    m2 = np.where(massless, L(1), mass2)
    invTot = np.where(massless, L(0), 1 / (mass1 + m2))                              # Ref :338 (pairInvTotalMass)
    dotvr2 = np.where(massless, L(0), (vel2 * bondDir).sum(1))
    vp2 = vel2 - bondDir * dotvr2[:, None]
    vbCMass = np.where(massless, L(0), (mass1 * dotvr1 + mass2 * dotvr2) * invTot)   # Ref :342 (a massless parent: Ref :323-334)
    c1, c2 = dotvr1 - vbCMass, dotvr2 - vbCMass
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.abs(c1 - c2)
        dt_raw = np.where(gap != 0, deltaR / gap, np.inf) / dt                       # Ref :345-346 (:326-327)
        deltaT = np.where(gap != 0, deltaR / gap, dt)
        if mutant != "no_clamp":
            deltaT = np.where(deltaT > dt, dt, deltaT)                               # Ref :347-348
        vBond = hws / np.sqrt(mass2 if mutant == "swap_masses_in_vbond" else mass1)   # Ref :349
        f1 = np.where(massless, L(1), mass2 * invTot)
        f2 = mass1 * invTot
        n1 = -c1 * vBond * f1 / np.abs(c1)                                           # Ref :350 (:330)
        n2 = np.where(massless, L(0), -c2 * vBond * f2 / np.abs(c2))                 # Ref :351
    dr1 = -deltaR * f1 + deltaT * n1                                                 # Ref :352 (:331)
    dr2 = deltaR * f2 + deltaT * n2                                                  # Ref :353
    n1, n2 = n1 + vbCMass, n2 + vbCMass
    hit = out if mutant != "no_wall" else np.zeros_like(out)
    move2 = hit & ~massless if mutant != "parent_not_updated" else np.zeros_like(out)
    pos[p1[hit]] += (bondDir * dr1[:, None])[hit]
    vel[p1[hit]] = (vp1 + bondDir * n1[:, None])[hit]
    pos[p2[move2]] += (bondDir * dr2[:, None])[move2]
    vel[p2[move2]] = (vp2 + bondDir * n2[:, None])[move2]
    info = dict(ratio=(r / max_dist).astype(np.float64), out=np.asarray(out), dt_raw=np.asarray(dt_raw, np.float64),
                dotvr1=c1.astype(np.float64), dotvr2=c2.astype(np.float64),
                vperp=np.sqrt(((vp1 - vp2) ** 2).sum(1)).astype(np.float64))
    return pos.astype(np.float64), vel.astype(np.float64), info


# (name, pairs dealt to it out of 8, Drude-parent distance / wall, radial and tangential relative speed x dt / wall).  With
# dt = 1 fs and a 0.02 nm wall a speed of 1 here is 20 nm/ps.  What a pair IS in a given begin is read off the reference's state
# before the wall (wall_classes): the Drude thermostat takes a few per cent off these speeds per half step and the kicks add
# ~0.25 nm/ps each.  The slowest class moves at 2 nm/ps: the parent's centred radial speed is m_D / M of the Drude's, and that
# too must stay clear of zero by the margin tests/test_hardwall.py asks for.
HOT_CLASSES = (("free", 1, 0.97, 0.15, 0.0),           # from just inside, fast: deltaT < dt
               ("clamped", 1, 1.35, 0.10, 0.0),        # starts outside, slow: deltaT clamped to dt
               ("approaching", 2, 1.40, -0.10, 0.0),   # outside, the Drude coming back: the reference turns it round all the same
               ("tangential", 1, 0.97, 0.15, 0.25),
               ("far", 1, 1.60, 0.10, 0.0),            # between 1.5 x and 2 x the wall
               ("late", 1, 0.80, 0.125, 0.0),          # delay = 0: crosses in the second step's begin (free there); delay = 1: stays inside
               ("late_tangential", 1, 0.80, 0.125, 0.25))
WALL_CLASSES = ("inside", "free", "clamped", "approaching", "tangential", "far")
TANGENTIAL_SPEED = 2.0     # nm/ps across the bond: above every thermal relative speed of the synthetic systems' pairs here
HOT_DRUDE_COUPLING = 0.05  # ps: these pairs are ~100 K hot against a 1 K bath; at the synthetic systems' 0.005 ps the Drude
                           # thermostat takes 80 % off their speed in the first half step, at this 3 %, then 5-10 %


def hot_wall_state(system, wall, seed, dt=0.001, sigma_force=200.0, num_forces=3, delay=0, beyond=None):
    """-> (positions, velocities, [forces]): the system's state with every Drude particle put where one rescale + half kick + drift
    takes its pair into one of HOT_CLASSES (dealt round robin over a seeded shuffle of the pairs; `beyond`: this pair goes past
    twice the wall instead), and `num_forces` explicit force arrays, N(0, sigma_force) kJ/mol/nm per component on massive
    particles (the harness' Drude spring would kick a 0.4 u particle at 0.02 nm by ~10 nm/ps and wipe the construction out).
    delay = 1: every Drude starts one drift further back, so the classes appear in the SECOND step's begin when the first step
    runs without a wall -- the only way to have a pair start that begin outside the wall (the deferred forms' first begin is the
    plain kernel; their own form is the second)."""
    rng = np.random.default_rng(seed)
    pos, vel = system.positions.copy(), system.velocities.copy()
    pd, pp = np.asarray(system.pair_drude), np.asarray(system.pair_parent)
    npair = len(pd)
    deal = np.repeat(np.arange(len(HOT_CLASSES)), [c[1] for c in HOT_CLASSES])
    kind = deal[np.arange(npair) % len(deal)][np.argsort(rng.permutation(npair))]
    dist, vr, vt = (np.array([c[k] for c in HOT_CLASSES], np.float64)[kind] for k in (2, 3, 4))
    if beyond is not None:
        dist[beyond], vr[beyond], vt[beyond] = 2.3, 0.10, 0.0
    u = rng.normal(size=(npair, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    t = np.cross(u, rng.normal(size=(npair, 3)))
    t /= np.linalg.norm(t, axis=1)[:, None]
    rel = u * (vr * rng.uniform(0.97, 1.03, npair))[:, None] + t * vt[:, None]       # relative velocity x dt / wall
    pos[pd] = pos[pp] + (u * dist[:, None] - 0.97 * delay * rel) * wall
    vel[pd] = vel[pp] + rel * (wall / dt)
    massive = (system.mass > 0)[:, None]
    forces = [rng.normal(0.0, sigma_force, pos.shape) * massive for _ in range(num_forces)]
    return pos, vel, forces


def wall_classes(info):
    """Which of WALL_CLASSES every pair is in, from hardwall_reference's decision quantities -> {name: bool[pairs]}.  A pair outside
    the wall is free or clamped, and may be approaching, tangential or far as well."""
    out = info["out"]
    return dict(inside=~out, free=out & (info["dt_raw"] < 1), clamped=out & (info["dt_raw"] > 1), approaching=out & (info["dotvr1"] < 0),
                tangential=out & (info["vperp"] > TANGENTIAL_SPEED), far=out & (info["ratio"] > 1.5) & (info["ratio"] < 2))


def wall_margins(info, vmax):
    """How far every decision of the wall is from its threshold, per pair and relative: |r / max_dist - 1|, |deltaT_raw / dt - 1|
    and both centred |dotvr| / max|v| for the pairs outside, |r / max_dist - 2| -> the smallest of each."""
    out = info["out"]
    big = np.array([np.inf])
    return dict(r=np.abs(info["ratio"] - 1).min(), twice=np.abs(info["ratio"] - 2).min(),
                deltaT=np.r_[big, np.abs(info["dt_raw"][out] - 1)].min(),
                dotvr1=np.r_[big, np.abs(info["dotvr1"][out]) / vmax].min(), dotvr2=np.r_[big, np.abs(info["dotvr2"][out]) / vmax].min())


def wall_sequence(o, system, walls, pos, vel, forces, dt, kT_drude, mutant=None):
    """The reference of tests/test_hardwall*.py, one step per entry of `walls` (the wall of that step's begin, 0 = none) from
    (pos, vel): per step k the oracle's propagate_nhc, half_kick(forces[k]) and drift, then hardwall_reference, then the oracle's
    half_kick(forces[k + 1]) and propagate_nhc.  -> per step a dict: pos, vel (directly after the begin), pre_pos, pre_vel (before
    the wall), info (with a wall).  The oracle's drift is the constrained form in either mode: x += dt v, v = (dt v) / dt
    (K :450-455), which is what the split entry points compute."""
    pos, vel = np.ascontiguousarray(pos, np.float64).copy(), np.ascontiguousarray(vel, np.float64).copy()
    steps = []
    for k, wall in enumerate(walls):
        f0, f1 = (np.ascontiguousarray(forces[j], np.float64) for j in (k, k + 1))
        o.propagate_nhc(vel); o.half_kick(vel, f0); o.drift(pos, vel)
        rec = dict(pre_pos=pos.copy(), pre_vel=vel.copy())
        if wall > 0:
            pos, vel, rec["info"] = hardwall_reference(pos, vel, system.mass, system.pair_drude, system.pair_parent, wall, dt, kT_drude, mutant)
        rec["pos"], rec["vel"] = pos.copy(), vel.copy()
        steps.append(rec)
        o.half_kick(vel, f1); o.propagate_nhc(vel)
    return steps


def wide_pairs(seed=13):
    """Eight waters and one 400-slot molecule whose 40 Drude particles sit 250-289 slots behind their parents: one 512-slot tile
    in which partner and self lie in different wavefronts of the work-group, so only __syncthreads() orders the LDS images."""
    rng = np.random.default_rng(seed)
    s, g, ng = synth.water_box(8)
    n0, nb = s.num_particles, 400
    mass = np.r_[s.mass, rng.uniform(6.0, 30.0, nb)]
    parents = n0 + np.arange(40)
    drudes = parents + 250 + np.arange(40)
    mass[drudes] = 0.4
    resid = np.r_[s.resid, np.full(nb, s.resid.max() + 1)].astype(np.int32)
    pos = np.r_[s.positions, rng.uniform(0.0, 0.7, (nb, 3))]
    return synth._finish(mass, np.r_[s.pair_drude, drudes].astype(np.int32), np.r_[s.pair_parent, parents].astype(np.int32), resid, pos,
                         np.zeros(n0 + nb, np.int32), 1, rng, 300.0, 1.0, "wide-pairs")


# ---- the cases tests/test_hardwall.py checks on the reference alone and tests/test_hardwall_gpu.py runs: one table for both ----
HOT_WALL, HOT_DT, HOT_SEED = 0.02, 0.001, 1
HOT_KT_DRUDE = synth.KB * 1.0
_DEFER, _RESIDENT, _WAVE, _GATHER = 2, 4, 8, 32          # include/drude_tgnh.h: TGNH_FLAG_*


def ragged(seed):
    mass, pd, pp, resid, group, ngroups, cons, sizes, first, rng = random_topology(seed)
    pos = rng.uniform(0.0, 3.0, (len(mass), 3))
    return synth._finish(mass, np.array(pd, np.int32), np.array(pp, np.int32), resid, pos, group, ngroups, rng, 300.0, 1.0, f"ragged{seed}")


WALL_SYSTEMS = {
    "water27": lambda: synth.water_box(27),                  # one tile; with TGNH_FLAG_WAVE_TILES three wave tiles, pattern-formed meta words
    "ragged6": lambda: ragged(6),                            # several 512-slot tiles, meta words read, Drude before and after its parent, pairs
                                                             # across wavefronts, two molecules longer than a tile (big_com beside the wall)
    "groups12": lambda: synth.many_groups(60, 6, 12),        # > 8 groups: KE bins in LDS behind the position image
    "wide": lambda: wide_pairs(),                            # partner and self in different wavefronts of one work-group
    "far": lambda: far_pairs(),                              # the tiles cannot hold it: the gather path by topology
}
SINGLE_SYSTEMS = ("water27", "wide")     # small boxes: kappa = max|x| / wall ~ 36, where float32 still resolves Drude - parent
# form -> flags, delay (hot_wall_state; 1: the first step runs without a wall and the form under test is the second begin), split
# (the constraint path's entry points), chains, systems, and what the handle must say it runs: resident_kernel(), step_path()[0]
HOT_FORMS = {
    "tile_kernel<S|K|D>": dict(flags=0, delay=0, split=False, chains=(1, 3), systems=("water27", "ragged6", "groups12", "wide"), kernel=None, path="tiled"),
    "tile_kernel<P|S|K|D>": dict(flags=_DEFER, delay=1, split=False, chains=(1, 3), systems=("water27", "ragged6", "groups12", "wide"), kernel=None, path="tiled"),
    "tile_kernel<MOVE>": dict(flags=0, delay=0, split=True, chains=(1,), systems=("water27", "ragged6", "wide"), kernel=None, path="tiled"),
    "step_kernel<STEP_PLAIN_BEGIN>": dict(flags=_RESIDENT, delay=0, split=False, chains=(1,), systems=("water27", "ragged6", "wide"), kernel="step_kernel", path="tiled"),
    "step_kernel<STEP_DEFER>": dict(flags=_RESIDENT | _DEFER, delay=1, split=False, chains=(1,), systems=("water27", "ragged6", "wide"), kernel="step_kernel", path="tiled"),
    "wstep_kernel": dict(flags=_RESIDENT | _DEFER | _WAVE, delay=1, split=False, chains=(1, 3), systems=("water27",), kernel="wstep_kernel", path="tiled"),
    "gather_update_kernel": dict(flags=_GATHER, delay=0, split=False, chains=(1, 3), systems=("water27", "ragged6", "groups12", "far"), kernel=None, path="gather"),
    "gather_update_kernel<MOVE>": dict(flags=_GATHER, delay=0, split=True, chains=(1,), systems=("water27", "far"), kernel=None, path="gather"),
}


def hot_form_cases():
    """-> [(form, system, mode, chains, precision)]: every case of tests/test_hardwall_gpu.py's form table"""
    out = []
    for form, d in HOT_FORMS.items():
        for sysname in d["systems"]:
            for chains in d["chains"]:
                if chains == 3 and sysname in ("groups12", "wide", "far"):      # (three links: once per kernel family is enough)
                    continue
                for mode in ("TGNH", "dualNH"):
                    for precision in ("single", "mixed", "double"):
                        if precision != "single" or sysname in SINGLE_SYSTEMS:
                            out.append((form, sysname, mode, chains, precision))
    return out


def hot_walls(delay, precision):
    """The wall of every step's begin, and the begins compared.  delay = 1: no wall in the first step, the second begin is the
    one.  delay = 0: both begins -- in single precision the first only: the pairs the first begin bounced leave it at the bath's
    thermal speed (0.14 nm/ps), a kick's size, and cross again in the second with centred radial speeds anywhere near zero: the
    margins single precision needs (tests/test_hardwall.py) cannot be had there by any choice of seed."""
    if delay:
        return (0.0, HOT_WALL), (1,)
    return ((HOT_WALL,), (0,)) if precision == "single" else ((HOT_WALL, HOT_WALL), (0, 1))


def hot_tolerances(precision, kappa):
    """(positions, velocities), both on rel_err.  double, mixed: 1e-12, include/drude_tgnh.h's figure for forms that agree to
    rounding.  single: 64 x 2^-24 for the ~40 dependent operations, the velocities' times kappa = max|x| / wall for the
    cancellation in Drude - parent, which the bond direction carries into every velocity the wall writes."""
    if precision == "single":
        return 64 * 2.0 ** -24, 64 * 2.0 ** -24 * kappa
    return 1e-12, 1e-12


class HotCase:
    """A system of WALL_SYSTEMS, its integrator (wall as given), oracle and hot state."""

    def __init__(self, sysname, mode, chains, delay, wall=HOT_WALL, seed=HOT_SEED, drude_temperature=1.0, beyond=None):
        self.system, g, ng = WALL_SYSTEMS[sysname]()
        self.group, self.ngroups = (g, ng) if mode == "TGNH" else (np.zeros_like(g), 1)
        self.mode, self.chains, self.drude_temperature = mode, chains, drude_temperature
        self.integrator = self.make_integrator(wall)
        self.pos, self.vel, self.forces = hot_wall_state(self.system, HOT_WALL, seed, HOT_DT, delay=delay, beyond=beyond)
        self.kappa = float(np.abs(self.pos).max() / HOT_WALL)

    def make_integrator(self, wall, drude_temperature=None):
        """a fresh one (a HipContext binds its integrator to itself)"""
        from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator
        td = self.drude_temperature if drude_temperature is None else drude_temperature
        it = DrudeTGNHIntegrator(300.0, 0.1, td, HOT_DRUDE_COUPLING, HOT_DT, 20, self.chains, True, True)
        it.setMaxDrudeDistance(wall)
        if self.mode == "TGNH":
            it._tempGroups = list(range(self.ngroups))
            it._particleTempGroup = np.ascontiguousarray(self.group, np.int32)
        return it

    def oracle(self):
        return make_oracle(self.system, self.group, self.ngroups, self.mode, self.integrator)

    def reference(self, walls, pos=None, vel=None, forces=None, mutant=None, kT_drude=None, oracle=None):
        kT_drude = synth.KB * self.drude_temperature if kT_drude is None else kT_drude
        return wall_sequence(oracle or self.oracle(), self.system, walls, self.pos if pos is None else pos, self.vel if vel is None else vel,
                             self.forces if forces is None else forces, HOT_DT, kT_drude, mutant)

    def members(self, mask):
        """slots of the pairs in `mask` (bool per pair), Drude particles then parents"""
        return np.r_[np.asarray(self.system.pair_drude)[mask], np.asarray(self.system.pair_parent)[mask]]
