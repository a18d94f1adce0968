"""The library's DrudeForce, bonded forces and NonbondedForce past one trip of the grid: the systems
tests/test_library_forces_at_size_gpu.py runs, and the shapes they must have, asserted without a GPU.

drude_force_kernel, bonded_body, exception_body and the nonbonded cell, place and rank kernels walk their receivers with a
grid-stride loop in index_grid's grid, which is capped at 1024 work-groups of 256: beyond 262 144 receivers a thread takes the loop
again.  The work-group behind an energy launch gives each thread ceil(rows / 256) rows (row_chunk): beyond 256 rows a thread adds
several and the last thread with any has fewer.  The units' own tests stay below both; the systems here are past both.

 * DrudeForce    131 100 isotropic pairs of tests/test_drude_force_gpu.py's isotropic_system and 3 lone atoms: 262 200 receivers,
                 two trips (56 receivers in the second), 1024 rows, 4 a thread; five screened pairs, one between two rows of the
                 second trip, one between a row of the first and one of the second.
 * bonded        tests/test_bonded_forces.py's system in its thermal state, 490 times over on an 8 x 8 x 8 lattice of 5.5 nm (a
                 dyadic spacing: the collinear ions keep exact coordinates in every stored type): 353 780 slots, 262 640 receivers
                 -- not a multiple of 256 --, the rows of each table shuffled across the copies.
 * nonbonded     65^3 = 274 625 ions (not a multiple of 64) on a lattice of 0.25 nm jittered by 0.04 nm, cutoff 0.3 nm, about five
                 neighbours each; every pair of slots (2k, 2k + 1) an evaluated exception: 274 624 exception receivers; 54^3 cells,
                 40 439 rows of pair energy, 158 a thread.  The twin's pairs come from tests/test_nonbonded.py's search.

THE ENERGY GATE AT SIZE.  A unit's GATE is measured on a few hundred terms and does not account for a sum this long.  The standard
bound on a floating-point sum of m terms added in any order is (depth) x 2^-53 x the sum of the terms' magnitudes, depth the longest
chain of additions a term passes through.  sum_depth derives it from the order tgnh_rows_device.h documents: a thread adds the terms
of its receivers, trip after trip; a wavefront adds its lanes in log2(64) = 6 levels; a work-group its 4 wavefronts one after the
other; a thread of the final work-group its rows; then the wavefront and the work-group once more.  The gate at size is the unit's
GATE plus that, times the sum of the terms' magnitudes; it is held against the fp80 sum, never against the device."""
import numpy as np

from openmm_drudenose_amd.system import DrudeSystem
from test_bonded_forces import bonded_system, positions as bonded_positions, receivers as bonded_receivers
from test_nonbonded import cells_per_edge, searched_pairs, stored
from test_nonbonded_geometry import BLOCK, INDEX_GRID_CAP, index_grid, nb_chunk_cap, nb_pair_grid, row_chunk

ONE_TRIP = INDEX_GRID_CAP * BLOCK
_cache = {}


def trips(receivers):
    return -(-receivers // (index_grid(receivers) * BLOCK))


def sum_depth(terms_per_thread, rows):
    """the longest chain of additions between a term and the total: the thread's own, the wavefront sum, the wavefronts of a
    work-group, row_chunk's rows per thread, and the final work-group's wavefront sum and wavefronts"""
    wave, waves = int(np.log2(64)), BLOCK // 64 - 1
    return terms_per_thread + wave + waves + row_chunk(rows)[0] + wave + waves


# ---------------------------------------------------------------------------
# DrudeForce
# ---------------------------------------------------------------------------
DRUDE_PAIRS, DRUDE_LONE = 131_100, 3
SCREENED = ((0, 1, 1.3), (10, 11, 2.6), (131_098, 131_099, 1.3), (5, 131_090, 0.9), (131_080, 131_081, 0.0))      # (row, row, thole)


def drude_at_size():
    """-> DrudeSystem with its DrudeForce attached (isotropic rows and SCREENED)"""
    if "drude" not in _cache:
        from test_drude_force_gpu import isotropic_system         # (its builder, as that file uses it)
        s = isotropic_system(DRUDE_PAIRS, DRUDE_LONE, 21)
        f = s.drude_force
        for i, j, thole in SCREENED:
            f.addScreenedPair(i, j, thole)
        s.set_drude_force(f)
        _cache["drude"] = s
    return _cache["drude"]


def test_the_drude_system_is_past_one_trip():
    s = drude_at_size()
    particles, params, screened, thole = s.drude_force.tables()
    recv = np.unique(particles[particles >= 0])
    assert len(recv) == 2 * DRUDE_PAIRS > ONE_TRIP and len(recv) % BLOCK != 0 and trips(len(recv)) == 2
    assert index_grid(len(recv)) == INDEX_GRID_CAP and row_chunk(index_grid(len(recv)))[0] == 4
    assert len(screened) == len(SCREENED) and np.count_nonzero(thole == 0.0) == 1
    second = particles[screened, 0] >= ONE_TRIP                   # the Drude slot of a row: a receiver of the second trip
    assert second.all(1).any() and (second[:, 0] != second[:, 1]).any() and (~second).all(1).any()
    x = s.positions
    d = np.linalg.norm(x[particles[screened[:, 0], 1]] - x[particles[screened[:, 1], 1]], axis=1)
    assert (d < 0.41).sum() == 4 and d.max() > 5.0               # lattice neighbours, and one pair far apart
    assert s.num_particles == 2 * DRUDE_PAIRS + DRUDE_LONE


# ---------------------------------------------------------------------------
# bonded forces
# ---------------------------------------------------------------------------
BONDED_COPIES, BONDED_SPACING = 490, 5.5


def bonded_at_size():
    """-> (DrudeSystem, tables as BondedForces takes them)"""
    if "bonded" not in _cache:
        s, tables, info = bonded_system()
        n, R = s.num_particles, BONDED_COPIES
        rng = np.random.default_rng(31)
        r = np.arange(R)
        shift = (np.stack([r // 64, (r // 8) % 8, r % 8], 1) - 3.5) * BONDED_SPACING
        x = (bonded_positions("thermal")[None, :, :] + shift[:, None, :]).reshape(-1, 3)
        out = []
        for table in tables:
            order = rng.permutation(R * len(table[0]))            # the rows of a table across all copies, out of slot order
            atoms = (table[0][None, :, :] + (n * r)[:, None, None]).reshape(-1, table[0].shape[1]).astype(np.int32)
            rest = [np.tile(a, (R,) + (1,) * (a.ndim - 1)) for a in table[1:]]
            out.append(tuple(a[order] for a in [atoms] + rest))
        big = DrudeSystem(mass=np.tile(s.mass, R), pair_drude=(s.pair_drude[None, :] + (n * r)[:, None]).ravel(),
                          pair_parent=(s.pair_parent[None, :] + (n * r)[:, None]).ravel(),
                          resid=(s.resid[None, :] + ((s.resid.max() + 1) * r)[:, None]).ravel(), positions=x, velocities=np.zeros_like(x),
                          name=f"{R} copies of the bonded system")
        _cache["bonded"] = (big, tuple(out))
    return _cache["bonded"]


def test_the_bonded_system_is_past_one_trip():
    s, tables = bonded_at_size()
    small, small_tables, info = bonded_system()
    recv = bonded_receivers(tables)
    assert len(recv) == BONDED_COPIES * len(bonded_receivers(small_tables)) > ONE_TRIP and len(recv) % BLOCK != 0 and trips(len(recv)) == 2
    assert index_grid(len(recv)) == INDEX_GRID_CAP > BLOCK and row_chunk(index_grid(len(recv)))[0] == 4
    for t, t0 in zip(tables, small_tables):
        assert len(t[0]) == BONDED_COPIES * len(t0[0]) and np.any(np.diff(t[0][:, 0]) < 0) and t[0].max() < s.num_particles
        assert np.abs(np.diff(t[0][:, 0])).max() > ONE_TRIP       # neighbouring rows from either end of the slots
    # the copies' shifts are dyadic: the collinear ions stay exact in every stored type, in every copy
    n = small.num_particles
    for precision in ("double", "mixed", "single"):
        x = stored(s.positions, precision)["x"]
        assert np.array_equal(x.reshape(BONDED_COPIES, n, 3)[:, list(info["collinear_slots"])], s.positions.reshape(BONDED_COPIES, n, 3)[:, list(info["collinear_slots"])])
    assert np.abs(s.positions).max() < 22.0


# ---------------------------------------------------------------------------
# NonbondedForce
# ---------------------------------------------------------------------------
NB_EDGE, NB_SPACING, NB_JITTER, NB_CUTOFF, NB_DIELECTRIC, NB_SEED = 65, 0.25, 0.04, 0.3, 78.3, 41
NB_BOX = (NB_EDGE * NB_SPACING,) * 3


def nonbonded_at_size():
    """-> (DrudeSystem of plain ions, table as NonbondedForces takes it)"""
    if "nonbonded" not in _cache:
        rng = np.random.default_rng(NB_SEED)
        m = NB_EDGE
        idx = np.arange(m ** 3)
        site = np.stack([idx // (m * m), (idx // m) % m, idx % m], 1)
        x = (site + 0.5) * NB_SPACING + rng.uniform(-NB_JITTER, NB_JITTER, (len(idx), 3))
        n = len(x)
        par = np.stack([np.where(site.sum(1) % 2 == 0, 0.5, -0.5), np.full(n, 0.2), np.full(n, 0.3)], 1)
        k = np.arange(n // 2)
        ep = np.stack([2 * k, 2 * k + 1], 1).astype(np.int32)
        ex = np.stack([0.5 * par[ep[:, 0], 0] * par[ep[:, 1], 0], np.full(len(k), 0.2), np.full(len(k), 0.15)], 1)
        s = DrudeSystem(mass=np.full(n, 23.0), pair_drude=np.zeros(0, np.int32), pair_parent=np.zeros(0, np.int32), resid=np.arange(n, dtype=np.int32),
                        positions=x, velocities=np.zeros_like(x), name=f"{n} ions on a jittered lattice")
        _cache["nonbonded"] = (s, (2, NB_CUTOFF, NB_DIELECTRIC, par, ep, ex))
    return _cache["nonbonded"]


def nonbonded_pairs(precision="mixed"):
    """the searched pairs of the positions as a precision stores them -> ((a, b), gap)"""
    if ("pairs", precision) not in _cache:
        s, table = nonbonded_at_size()
        _cache["pairs", precision] = searched_pairs(stored(s.positions, precision)["x"], table, NB_BOX)
    return _cache["pairs", precision]


def test_the_nonbonded_system_is_past_one_trip():
    s, table = nonbonded_at_size()
    n = s.num_particles
    assert n == NB_EDGE ** 3 > ONE_TRIP and n % 64 != 0 and NB_EDGE >= 64 and trips(n) == 2
    ev = (table[5][:, 0] != 0) | (table[5][:, 2] != 0)
    recv = len(np.unique(table[4][ev]))
    assert ev.all() and recv > ONE_TRIP and trips(recv) == 2 and index_grid(recv) == INDEX_GRID_CAP
    nc = cells_per_edge(NB_BOX, NB_CUTOFF)
    ncells = int(np.prod(nc))
    assert nc == (54, 54, 54) and ncells > BLOCK and NB_CUTOFF <= 0.5 * min(NB_BOX)
    chunk, r0, r1 = row_chunk(nb_pair_grid(n, ncells))
    assert nb_pair_grid(n, ncells) == 40_439 and chunk == 158 and 0 < (r1 - r0).min() < chunk                 # a ragged end
    (a, b), gap = nonbonded_pairs()
    assert gap >= 1e-9, gap                                       # nobody at the cutoff, with this seed
    per_slot = np.bincount(a, minlength=n)
    print(f"nonbonded at size: {len(a)} ordered pairs inside the cutoff, {per_slot.mean():.2f} a slot (most {per_slot.max()}); nearest to the cutoff {gap:.2e} of rc^2")
    assert 5.0 < per_slot.mean() < 9.0 and per_slot.min() >= 1
    # the exceptions' partners are lattice neighbours, except where a pair straddles the end of a lattice row
    d = np.linalg.norm(s.positions[table[4][:, 0]] - s.positions[table[4][:, 1]], axis=1)
    assert np.median(d) < 0.3 and (d < 0.35).mean() > 0.98 and d.min() > 0.15
