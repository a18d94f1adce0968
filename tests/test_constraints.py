"""CPU tests of the direct constraint solver's host side (tgnh_set_constraint_clusters on a host-only handle, split_clusters) and of the
yardstick tests/test_constraints_gpu.py measures the kernels against: the oracle's SHAKE, converged.

The states of the GPU tests are built HERE (`state`), once per (shape, precision), and never changed:
 * positions: the system's own, shifted by (3.1, -2.7, 0.4) nm so that coordinates are not small, split into the stored types
   (single / mixed: float32, mixed with a float32 correction);
 * displacements: dt v' with dt = 1 fs and v' thermal at 300 K, drawn per massive atom WITHOUT regard to the constraints -- much
   harder than a real step, whose velocities already satisfy them; velocities: another such draw.  Fixed seeds.
The oracle is fed the stored values upcast to fp64, as the device reads them.  Its SHAKE gives up after 500 sweeps with an error;
a GPU test that compared against a reference that gave up would prove nothing, so the tests here ask that it converges for every
state, at the tolerances the GPU tests use (1e-14 positions, 1e-12 velocities), and that the converged bonds are at their lengths."""
import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator, HostTopology, TgnhError, split_clusters
from openmm_drudenose_amd.system import DrudeSystem
from helpers import make_oracle

SHIFT = np.array([3.1, -2.7, 0.4])
DT = 0.001                       # ps
TEMPERATURE = 300.0
SHAKE_TOL, RATE_TOL = 1e-14, 1e-12
PRECISIONS = ("double", "mixed", "single")
PAIRS = DrudeSystem.PAIRS
XH3_GEOM = np.array([[0.0, 0.0, 0.0], [0.109, 0.0, 0.0], [-0.036, 0.103, 0.0], [-0.036, -0.051, 0.089]])


def _plain(mass, resid, pos, atoms, dist, name, pair_drude=(), pair_parent=()):
    s = DrudeSystem(mass=np.asarray(mass, np.float64), pair_drude=np.asarray(pair_drude, np.int32), pair_parent=np.asarray(pair_parent, np.int32),
                    resid=np.asarray(resid, np.int32), positions=np.asarray(pos, np.float64), velocities=np.zeros((len(mass), 3)), name=name)
    s.set_clusters(atoms, dist)
    return s, np.zeros(len(mass), np.int32), 1


def xh3_cluster(first):
    """one X-H3 cluster on the slots first .. first + 3: three bonds from atom 0"""
    d = np.linalg.norm(XH3_GEOM[1:] - XH3_GEOM[0], axis=1)
    return [first, first + 1, first + 2, first + 3], [d[0], d[1], d[2], 0.0, 0.0, 0.0]


def xh3_system():
    """12 slots: three X-H3 clusters (4 atoms, 3 constraints each)"""
    pos = np.concatenate([XH3_GEOM + np.array([0.4 * m, 0.0, 0.0]) for m in range(3)])
    cl = [xh3_cluster(4 * m) for m in range(3)]
    return _plain([12.011, 1.008, 1.008, 1.008] * 3, np.repeat(np.arange(3), 4), pos, [c[0] for c in cl], [c[1] for c in cl], "xh3")


def mixed_system():
    """Three rigid waters (slots 0..14), two X-H (15..18) and two X-H3 (19..26) in one system, its clusters handed over in REVERSE
    slot order: what the sort at set time is for."""
    w = synth.water_box(3, rigid=True)[0]
    n0 = w.num_particles
    mass = np.r_[w.mass, [12.011, 1.008] * 2, [12.011, 1.008, 1.008, 1.008] * 2]
    xh = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.101]])
    pos = np.concatenate([w.positions] + [xh + np.array([0.5 * m, 1.0, 0.0]) for m in range(2)] + [XH3_GEOM + np.array([0.5 * m, 2.0, 0.0]) for m in range(2)])
    resid = np.r_[w.resid, 3 + np.repeat(np.arange(2), 2), 5 + np.repeat(np.arange(2), 4)]
    atoms = [list(a) for a in w.cluster_atoms] + [[n0 + 2 * m, n0 + 2 * m + 1, -1, -1] for m in range(2)]
    dist = [list(d) for d in w.cluster_dist] + [[0.101, 0, 0, 0, 0, 0]] * 2
    for m in range(2):
        a, d = xh3_cluster(n0 + 4 + 4 * m)
        atoms.append(a); dist.append(d)
    s, g, ng = _plain(mass, resid, pos, atoms[::-1], dist[::-1], "water+xh+xh3, reversed", w.pair_drude, w.pair_parent)
    s.set_virtual_sites(w.site_atoms, w.site_weights)
    return s, g, ng


SHAPES = {
    "water1": lambda: synth.water_box(1, rigid=True),             # one lane
    "water65": lambda: synth.water_box(65, rigid=True),           # a second wavefront
    "water257": lambda: synth.water_box(257, rigid=True),         # a second work-group
    "il2": lambda: synth.ionic_liquid(2, constrained=True),       # 20 clusters of 1 and 2 constraints, on non-consecutive slots
    "xh3": xh3_system,                                            # 4 atoms, 3 constraints
    "mixed-reversed": mixed_system,                               # all kinds, given in reverse order
}
_cache = {}


def shape(name):
    if name not in _cache:
        _cache[name] = SHAPES[name]()
    return _cache[name]


def integrator():
    return DrudeTGNHIntegrator(TEMPERATURE, 0.1, 1.0, 0.005, DT, 20, 1, True, True)


def _thermal(rng, mass):
    v = np.zeros((len(mass), 3))
    m = mass > 0
    v[m] = rng.normal(0.0, 1.0, (int(m.sum()), 3)) * np.sqrt(synth.KB * TEMPERATURE / mass[m])[:, None]
    return v


def state(name, precision):
    """The stored arrays of a shape in a precision and their fp64 reading -> dict: posq [N,3] (float32 / float64), corr [N,3] float32
    or None, delta and vel [N,3] in the type of posDelta / velm (float32 in single), x / d / v: the same three as the device reads
    them, in fp64.  Built once; callers copy what they change."""
    key = (name, precision, "state")
    if key not in _cache:
        s = shape(name)[0]
        rng = np.random.default_rng(20241 + sorted(SHAPES).index(name))
        x = s.positions + SHIFT
        delta, vel = DT * _thermal(rng, s.mass), _thermal(rng, s.mass)
        real = np.float64 if precision == "double" else np.float32
        mixed = np.float32 if precision == "single" else np.float64
        posq = x.astype(real)
        corr = (x - posq.astype(np.float64)).astype(np.float32) if precision == "mixed" else None
        st = dict(posq=posq, corr=corr, delta=delta.astype(mixed), vel=vel.astype(mixed))
        st["x"] = posq.astype(np.float64) + (corr.astype(np.float64) if corr is not None else 0.0)
        st["d"], st["v"] = st["delta"].astype(np.float64), st["vel"].astype(np.float64)
        for a in st.values():
            if a is not None:
                a.setflags(write=False)
        _cache[key] = st
    return _cache[key]


def reference(name, precision):
    """The oracle's converged SHAKE on a state -> (delta', vel') in fp64: SHAKE at 1e-14 on the displacements, the velocity stage at
    1e-12 on the velocities.  Raises OracleError if either gives up.  Computed once."""
    key = (name, precision, "reference")
    if key not in _cache:
        s, g, ng = shape(name)
        st = state(name, precision)
        o = make_oracle(s, g, ng, "TGNH", integrator())
        x, d, v = (np.ascontiguousarray(st[k]).copy() for k in ("x", "d", "v"))
        o.shake_positions(x, d, SHAKE_TOL)
        o.shake_velocities(x, v, RATE_TOL)
        d.setflags(write=False); v.setflags(write=False)
        _cache[key] = (d, v)
    return _cache[key]


def constraints_of(s):
    """(i, j, d, cluster) of every constraint of a system's clusters"""
    out = []
    for k, (a, b) in enumerate(PAIRS):
        m = np.flatnonzero(s.cluster_dist[:, k] > 0)
        out.append(np.stack([s.cluster_atoms[m, a], s.cluster_atoms[m, b], m], 1))
    ijc = np.concatenate(out)
    dist = np.concatenate([s.cluster_dist[s.cluster_dist[:, k] > 0, k] for k in range(6)])
    return ijc[:, 0], ijc[:, 1], dist, ijc[:, 2]


def bond_violation(s, x, delta):
    """largest |d'^2 - d^2| / d^2 over the constraints, the new bond vector formed as (x_i - x_j) + (delta_i - delta_j) in fp64"""
    i, j, d, _ = constraints_of(s)
    sv = (x[i] - x[j]) + (delta[i] - delta[j])
    return float((np.abs((sv * sv).sum(1) - d * d) / (d * d)).max())


def rate_violation(s, x, vel, weighted=True):
    """largest |r . (v_i - v_j)| / r^2 / sqrt(w_i + w_j) over the constraints (weighted=False: without the last divisor)"""
    i, j, _, _ = constraints_of(s)
    r, dv = x[i] - x[j], vel[i] - vel[j]
    rate = np.abs((r * dv).sum(1)) / (r * r).sum(1)
    return float((rate / np.sqrt(1.0 / s.mass[i] + 1.0 / s.mass[j]) if weighted else rate).max())


# ---------------------------------------------------------------------------
# the yardstick's own condition
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_oracle_converges_on_every_state(name, precision, oracle_lib):
    s = shape(name)[0]
    st = state(name, precision)
    assert bond_violation(s, st["x"], st["d"]) > 1e-3 and rate_violation(s, st["x"], st["v"]) > 1e-2      # the draw ignores the constraints
    d, v = reference(name, precision)                                   # (an OracleError "did not converge" fails the test here)
    bv, rv = bond_violation(s, st["x"], d), rate_violation(s, st["x"], v, weighted=False)
    print(f"oracle SHAKE {name} {precision}: bonds {bv:.2e} rates {rv:.2e}")
    assert bv <= 1e-13
    assert rv <= 2 * RATE_TOL        # the stage's own criterion |r . dv| / r^2 <= tol, held by every constraint in its last sweep; re-evaluated here in another order of operations
    untouched = np.setdiff1d(np.arange(s.num_particles), s.cluster_atoms[s.cluster_atoms >= 0])
    assert np.array_equal(d[untouched], st["d"][untouched]) and np.array_equal(v[untouched], st["v"][untouched])


# ---------------------------------------------------------------------------
# tgnh_set_constraint_clusters on a host-only handle
# ---------------------------------------------------------------------------
def host(s):
    return HostTopology(s, integrator())


def refused(top, atoms, dist, status, match):
    with pytest.raises(TgnhError, match=match) as e:
        top.set_constraint_clusters(atoms, dist)
    assert e.value.status == status


def test_accepted_tables_and_the_count():
    for make, k in ((lambda: synth.water_box(2, rigid=True), 2), (lambda: synth.ionic_liquid(1, constrained=True), 10), (xh3_system, 3),
                    (mixed_system, 7)):
        s = make()[0]
        top = host(s)
        assert top.num_constraint_clusters() == 0
        top.set_constraint_clusters(s.cluster_atoms, s.cluster_dist)
        assert top.num_constraint_clusters() == k == len(s.cluster_atoms)
        dof = top.dof()[0].copy()
        top.set_constraint_clusters(s.cluster_atoms[:1], s.cluster_dist[:1])          # a second table replaces the first
        assert top.num_constraint_clusters() == 1
        top.set_constraint_clusters(np.zeros((0, 4), np.int32), np.zeros((0, 6)))     # n = 0 clears it
        assert top.num_constraint_clusters() == 0
        assert np.array_equal(top.dof()[0], dof)                                      # the degrees of freedom are the descriptor's
        top.close()
    il = synth.ionic_liquid(1, constrained=True)[0]
    ncons = (il.cluster_dist > 0).sum(1)
    assert set(ncons) == {1, 2} and np.any(np.diff(il.cluster_atoms[:, :2], axis=1) > 1)      # 1 and 2 constraints, non-consecutive slots


def test_refusals():
    s = xh3_system()[0]
    top = host(s)
    a, d = s.cluster_atoms.copy(), s.cluster_dist.copy()
    lib = top.lib
    assert lib.tgnh_set_constraint_clusters(top.h, -1, None, None) == _lib.ERR_ARG
    assert lib.tgnh_set_constraint_clusters(top.h, 1, None, None) == _lib.ERR_ARG
    assert lib.tgnh_get_num_constraint_clusters(top.h, None) == _lib.ERR_ARG
    assert lib.tgnh_set_constraint_clusters(None, 0, None, None) == _lib.ERR_ARG

    def with_(ai=None, di=None):
        a2, d2 = a.copy(), d.copy()
        if ai is not None:
            a2[ai[0], ai[1]] = ai[2]
        if di is not None:
            d2[di[0], di[1]] = di[2]
        return a2, d2
    refused(top, *with_(ai=(1, 2, 12)), _lib.ERR_ARG, "cluster 1.*out of range")
    refused(top, *with_(ai=(1, 2, -2)), _lib.ERR_ARG, "cluster 1.*out of range")
    refused(top, *with_(ai=(2, 3, 8)), _lib.ERR_ARG, "cluster 2 lists atom 8 twice")
    refused(top, *with_(ai=(2, 3, 1)), _lib.ERR_ARG, "cluster 2 and cluster 0 share atom 1")
    refused(top, *with_(ai=(0, 3, -1)), _lib.ERR_ARG, "cluster 0.*unused atom")
    refused(top, *with_(di=(1, 0, -0.1)), _lib.ERR_ARG, "cluster 1.*negative or not finite")
    refused(top, *with_(di=(1, 1, np.nan)), _lib.ERR_ARG, "negative or not finite")
    refused(top, *with_(di=(1, 1, np.inf)), _lib.ERR_ARG, "negative or not finite")
    a0, d0 = a.copy(), d.copy()
    d0[2] = 0.0
    refused(top, a0, d0, _lib.ERR_ARG, "cluster 2 holds no constraint")
    refused(top, *with_(di=(1, 3, 0.178)), _lib.ERR_UNSUPPORTED, "cluster 1 holds 4 constraints.*iterative solver")
    assert top.num_constraint_clusters() == 0                                           # a refused table changes nothing
    top.set_constraint_clusters(a, d)
    refused(top, *with_(di=(1, 3, 0.178)), _lib.ERR_UNSUPPORTED, "cluster 1")
    assert top.num_constraint_clusters() == 3
    top.close()
    w = synth.water_box(2, rigid=True)[0]                        # O, D, H1, H2, M: the M site has no mass
    top = host(w)
    aw, dw = w.cluster_atoms.copy(), w.cluster_dist.copy()      # molecule 1: (5, 7, 8, -1), its M site is slot 9
    aw[1, 2] = 9
    refused(top, aw, dw, _lib.ERR_UNSUPPORTED, "cluster 1: constrained atom 9 has no mass")
    aw[1] = (5, 7, 8, 9)                                         # ... a massless member that no constraint names is nobody's business
    top.set_constraint_clusters(aw, dw)
    assert top.num_constraint_clusters() == 2
    # the apply calls on a host-only handle
    assert top.lib.tgnh_apply_constraints(top.h, 1e-5, None) == _lib.ERR_STATE
    assert top.lib.tgnh_apply_velocity_constraints(top.h, 1e-5, None) == _lib.ERR_STATE
    top.close()


def test_split_clusters():
    s = mixed_system()[0]
    four = ([30, 31, 32, 33], [0.1, 0.1, 0.1, 0.16, 0.0, 0.0])                  # 4 atoms, 4 distances
    five = ([40, 41, 42, 43], [0.1, 0.1, 0.1, 0.16, 0.16, 0.0])
    atoms = np.array([four[0]] + [list(a) for a in s.cluster_atoms[:4]] + [five[0]] + [list(a) for a in s.cluster_atoms[4:]], np.int32)
    dist = np.array([four[1]] + [list(d) for d in s.cluster_dist[:4]] + [five[1]] + [list(d) for d in s.cluster_dist[4:]])
    (da, dd), (ra, rd) = split_clusters(atoms, dist)
    assert np.array_equal(da, s.cluster_atoms) and np.array_equal(dd, s.cluster_dist)          # order kept
    assert np.array_equal(ra, np.array([four[0], five[0]], np.int32)) and np.array_equal(rd, np.array([four[1], five[1]]))
    assert len(da) + len(ra) == len(atoms) and da.dtype == np.int32 and dd.dtype == np.float64
    assert set((dd > 0).sum(1)) == {1, 3} and np.all((rd > 0).sum(1) > 3)
    (da, dd), (ra, rd) = split_clusters(np.zeros((0, 4), np.int32), np.zeros((0, 6)))
    assert da.shape == ra.shape == (0, 4) and dd.shape == rd.shape == (0, 6)
    # what the library says to the side split_clusters keeps from it
    top = host(xh3_system()[0])
    refused(top, np.array([[0, 1, 2, 3]], np.int32), np.array([four[1]]), _lib.ERR_UNSUPPORTED, "4 constraints")
    top.close()
    import drudetgnhplugin
    assert drudetgnhplugin.split_clusters is split_clusters
