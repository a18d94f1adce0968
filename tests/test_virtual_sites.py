"""CPU tests of the library's virtual-site stage: tgnh_set_virtual_sites' checks on a host-only handle, and the yardstick
tests/test_virtual_sites_gpu.py measures the kernels against.

The yardstick is `placement` and `transpose` below: OpenMM's four site kinds and the transposes of their Jacobians, written from the
formulas of include/drude_tgnh.h over arrays of any floating type.  Run on numpy longdouble (fp80) they are THE REFERENCE; run on
float64 they are THE TWIN, whose every operation numpy rounds on its own, in the order written -- what the device is asked to
reproduce bit for bit for the two average kinds.  The reference is itself checked here: every transpose against central finite
differences of its own placement in fp80, and the invariants sum of shares = f and sum x_m x share_m = x_site x f.

The table and the states of the GPU tests are built HERE (`site_system`, `state`), once, and never changed: 103 rounds of three
molecules -- a five-site water (O, H1, H2 and two out-of-plane lone pairs on the same three parents), a fragment A, B, C with a
local-coordinates lone pair on (A, B, C) and a two-particle average on (A, B), and a four-site water whose three-particle average M
comes BEFORE its parents -- 515 sites = 2 x 256 + 3 on 1442 slots (padded 1472), the table shuffled; molecule centres uniform in
+-7.5 nm, split into the stored types as Context::setPositions does; forces normal, 1e3 kJ/mol/nm, on every slot.

THE GPU MARGIN.  The largest difference between twin and reference over the three states (placements, and shares of the states'
forces), out-of-plane and local-coordinates sites only, relative to the largest component (by magnitude) of the result in that site
-- the site's coordinates, or its three shares --, measured by test_the_margin_between_twin_and_reference: placements 2.98e-16,
shares 8.68e-15 (a local-coordinates frame 0.1 nm across is a difference of coordinates near 8 nm: their roundings, 2^-53 x 8 nm, are
1e-14 of it); MEASURED_MARGIN is the larger, rounded up.  The GPU gate for those two kinds is 16 x MEASURED_MARGIN: room for
another order of operations and for contraction.  It comes from the reference and the number format, never from the device."""
import numpy as np
import pytest

from openmm_drudenose_amd import _lib
from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator, HostTopology, TgnhError
from openmm_drudenose_amd.system import DrudeSystem

TWO, THREE, PLANE, LOCAL = _lib.SITE_TWO_AVERAGE, _lib.SITE_THREE_AVERAGE, _lib.SITE_OUT_OF_PLANE, _lib.SITE_LOCAL_COORDINATES
PRECISIONS = ("double", "mixed", "single")
BLOCK = 256                      # csrc/tgnh_internal.h
ROUNDS = 103
MEASURED_MARGIN = 8.7e-15
GATE = 16 * MEASURED_MARGIN
FIXED = 4294967296.0
_cache = {}


# ---------------------------------------------------------------------------
# the four kinds, over arrays [S, 3] of one floating type (parents x1, x2, x3; parameters p [S, 12]; forces f)
# ---------------------------------------------------------------------------
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _dot(a, b):
    return ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2])[:, None]


def _weighted(w, x1, x2, x3):
    return (w[:, [0]] * x1 + w[:, [1]] * x2) + w[:, [2]] * x3


def _frame(p, x1, x2, x3):
    a, b = _weighted(p[:, 3:6], x1, x2, x3), _weighted(p[:, 6:9], x1, x2, x3)
    c = _cross(a, b)
    one = p.dtype.type(1)
    inv_a, inv_c = one / np.sqrt(_dot(a, a)), one / np.sqrt(_dot(c, c))
    X, Z = inv_a * a, inv_c * c
    return a, b, X, _cross(Z, X), Z, inv_a, inv_c


def placement(kind, x1, x2, x3, p):
    """the sites of one kind -> [S, 3]"""
    if kind == TWO:
        return p[:, [0]] * x1 + p[:, [1]] * x2
    if kind == THREE:
        return _weighted(p[:, 0:3], x1, x2, x3)
    if kind == PLANE:
        r12, r13 = x2 - x1, x3 - x1
        return ((x1 + p[:, [0]] * r12) + p[:, [1]] * r13) + p[:, [2]] * _cross(r12, r13)
    a, b, X, Y, Z, inv_a, inv_c = _frame(p, x1, x2, x3)
    return ((_weighted(p[:, 0:3], x1, x2, x3) + p[:, [9]] * X) + p[:, [10]] * Y) + p[:, [11]] * Z


def transpose(kind, x1, x2, x3, p, f):
    """the parents' shares of the forces f on the sites of one kind -> [3][S, 3] (a two-particle site: its third share is zero)"""
    if kind in (TWO, THREE):
        return [p[:, [m]] * f if m < (2 if kind == TWO else 3) else np.zeros_like(f) for m in range(3)]
    if kind == PLANE:
        r12, r13 = x2 - x1, x3 - x1
        f2 = p[:, [0]] * f + p[:, [2]] * _cross(r13, f)
        f3 = p[:, [1]] * f - p[:, [2]] * _cross(r12, f)
        return [(f - f2) - f3, f2, f3]
    a, b, X, Y, Z, inv_a, inv_c = _frame(p, x1, x2, x3)
    uX = p[:, [9]] * f + p[:, [10]] * _cross(f, Z)               # the gradients of f . site with respect to X and Z
    uZ = p[:, [11]] * f + p[:, [10]] * _cross(X, f)
    ta = inv_a * (uX - _dot(uX, X) * X)                          # ... through the two normalisations
    tc = inv_c * (uZ - _dot(uZ, Z) * Z)
    ga, gb = ta + _cross(b, tc), _cross(tc, a)                   # ... and through c = a x b
    return [(p[:, [m]] * f + p[:, [3 + m]] * ga) + p[:, [6 + m]] * gb for m in range(3)]


def evaluate(kinds, atoms, params, x, f, dtype):
    """A whole table in `dtype` -> (sites [S, 3], shares [S, 3, 3]) with the shares of the forces f[site]"""
    x, f, params = x.astype(dtype), f.astype(dtype), params.astype(dtype)
    sites, shares = np.zeros((len(kinds), 3), dtype), np.zeros((len(kinds), 3, 3), dtype)
    for kind in (TWO, THREE, PLANE, LOCAL):
        m = np.flatnonzero(kinds == kind)
        if not len(m):
            continue
        x1, x2, x3 = x[atoms[m, 1]], x[atoms[m, 2]], x[atoms[m, 3]]             # (a two-particle site: atoms[:, 3] = -1 reads a slot nobody uses)
        sites[m] = placement(kind, x1, x2, x3, params[m])
        for r, s in enumerate(transpose(kind, x1, x2, x3, params[m], f[atoms[m, 0]])):
            shares[m, r] = s
    return sites, shares


# ---------------------------------------------------------------------------
# the table and the states of the GPU tests
# ---------------------------------------------------------------------------
TIP5 = np.array([[0.0, 0.0, 0.0], [0.09572, 0.0, 0.0], [-0.023999, 0.092663, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
FRAG = np.array([[0.0, 0.0, 0.0], [0.1331, 0.011, -0.02], [-0.061, 0.118, 0.031], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
TIP4 = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.09572, 0.0, 0.0], [-0.023999, 0.092663, 0.0]])
PLANE_W = (-0.34490826, -0.34490826, 6.4437903)                  # TIP5P's lone pairs (the second one: -wc)
LOCAL_P = [1.0, 0.0, 0.0, -1.0, 0.5, 0.5, 0.0, -1.0, 1.0, -0.031, 0.012, 0.027]
LOCAL_Q = [0.7, 0.2, 0.1, -1.0, 0.75, 0.25, -0.5, -0.5, 1.0, 0.02, -0.015, 0.03]


def site_system():
    """-> (DrudeSystem with positions, kinds [S], atoms [S, 4], params [S, 12]): the table of the module docstring, shuffled"""
    if "system" in _cache:
        return _cache["system"]
    rng = np.random.default_rng(20250611)
    mass, pos, resid, kinds, atoms, params = [], [], [], [], [], []

    def row(kind, at, p):
        kinds.append(kind); atoms.append(at); params.append(list(p) + [0.0] * (12 - len(p)))
    n = 0
    for r in range(ROUNDS):
        for which, geom, m in ((0, TIP5, [15.9994, 1.008, 1.008, 0.0, 0.0]), (1, FRAG, [12.011, 14.007, 15.9994, 0.0, 0.0]), (2, TIP4, [0.0, 15.9994, 1.008, 1.008])):
            rot = np.linalg.qr(rng.normal(size=(3, 3)))[0]
            pos.append(geom @ rot.T + rng.uniform(-7.5, 7.5, 3))
            mass += m
            resid += [3 * r + which] * len(m)
            if which == 0:
                row(PLANE, [n + 3, n, n + 1, n + 2], PLANE_W)
                row(PLANE, [n + 4, n, n + 1, n + 2], (PLANE_W[0], PLANE_W[1], -PLANE_W[2]))
            elif which == 1:
                row(LOCAL, [n + 3, n, n + 1, n + 2], LOCAL_P if r % 2 else LOCAL_Q)
                row(TWO, [n + 4, n, n + 1, -1], (0.36 + 0.001 * (r % 7), 0.64 - 0.001 * (r % 7)))
            else:
                row(THREE, [n, n + 1, n + 2, n + 3], (0.786646558, 0.106676721, 0.106676721))
            n += len(m)
    kinds, atoms, params = np.array(kinds, np.int32), np.array(atoms, np.int32), np.array(params)
    pos = np.concatenate(pos)
    pos[atoms[:, 0]] = evaluate(kinds, atoms, params, pos, np.zeros_like(pos), np.float64)[0]
    s = DrudeSystem(mass=np.array(mass), pair_drude=np.zeros(0, np.int32), pair_parent=np.zeros(0, np.int32), resid=np.array(resid, np.int32),
                    positions=pos, velocities=np.zeros_like(pos), name="five kinds of molecules, 515 sites")
    order = rng.permutation(len(kinds))
    out = (s, np.ascontiguousarray(kinds[order]), np.ascontiguousarray(atoms[order]), np.ascontiguousarray(params[order]))
    for a in out[1:]:
        a.setflags(write=False)
    _cache["system"] = out
    return out


def state(precision):
    """The stored arrays of the table's system in a precision and their fp64 reading -> dict: posq [N, 3] (float32 / float64), corr
    [N, 3] float32 or None, x: the positions as the device reads them (fp64), force: int64 [N, 3] fixed point, f = force / 2^32.  The
    sites' own coordinates are off their placements (the device is to put them there).  Built once; callers copy what they change."""
    key = ("state", precision)
    if key not in _cache:
        s = site_system()[0]
        rng = np.random.default_rng(977)
        x = s.positions + rng.normal(0.0, 0.003, s.positions.shape)
        real = np.float64 if precision == "double" else np.float32
        posq = x.astype(real)
        corr = (x - posq.astype(np.float64)).astype(np.float32) if precision == "mixed" else None
        force = np.rint(rng.normal(0.0, 1e3, x.shape) * FIXED).astype(np.int64)
        st = dict(posq=posq, corr=corr, force=force, f=force.astype(np.float64) / FIXED)
        st["x"] = posq.astype(np.float64) + (corr.astype(np.float64) if corr is not None else 0.0)
        for a in st.values():
            if a is not None:
                a.setflags(write=False)
        _cache[key] = st
    return _cache[key]


def results(precision, dtype):
    """evaluate() on a state, computed once per (precision, type) -> (sites, shares)"""
    key = ("results", precision, np.dtype(dtype).name)
    if key not in _cache:
        _, kinds, atoms, params = site_system()
        st = state(precision)
        out = evaluate(kinds, atoms, params, st["x"], st["f"], dtype)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def integrator():
    return DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)


# ---------------------------------------------------------------------------
# the table is what the GPU tests need it to be
# ---------------------------------------------------------------------------
def test_the_table_has_the_shapes_the_kernels_can_go_wrong_at():
    s, kinds, atoms, params = site_system()
    n, S = s.num_particles, len(kinds)
    assert S == 2 * BLOCK + 3 and (n + 31) // 32 * 32 > n
    assert set(kinds) == {TWO, THREE, PLANE, LOCAL} and np.any(np.diff(atoms[:, 0]) < 0)                 # all kinds, unsorted
    assert np.any(kinds[np.argsort(atoms[:, 0])][:-1] != kinds[np.argsort(atoms[:, 0])][1:])           # interleaved in slot order too
    assert np.any(atoms[kinds == THREE, 0] < atoms[kinds == THREE, 1:].min(1))                           # a site before its parents
    parents = atoms[:, 1:][atoms[:, 1:] >= 0]
    assert n - 1 in parents and n - 1 not in atoms[:, 0]                                                 # the last slot receives
    count = {k: np.bincount(atoms[kinds == k, 1:][atoms[kinds == k, 1:] >= 0], minlength=n) for k in (TWO, THREE, PLANE, LOCAL)}
    assert count[PLANE].max() == 2                                                                       # two out-of-plane sites on one parent
    assert np.any((count[TWO] > 0) & (count[LOCAL] > 0))                                                 # sites of two kinds on one parent
    assert len(np.unique(parents)) > BLOCK                                                               # more than one work-group of receivers
    for precision in PRECISIONS:
        st = state(precision)
        assert 6.0 < np.abs(st["x"]).max() < 8.0 and np.isfinite(st["x"]).all()
        if precision == "mixed":
            assert np.count_nonzero(st["corr"]) > 0.9 * st["corr"].size
    w = params[kinds == LOCAL]
    assert np.abs(w[:, 0:3].sum(1) - 1).max() < 1e-15 and np.abs(w[:, 3:6].sum(1)).max() < 1e-15 and np.abs(w[:, 6:9].sum(1)).max() < 1e-15
    assert np.abs(params[kinds == TWO, :2].sum(1) - 1).max() < 1e-15 and np.abs(params[kinds == THREE, :3].sum(1) - 1).max() < 1e-9


# ---------------------------------------------------------------------------
# the reference checked against itself
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_every_transpose_against_finite_differences_of_its_placement(precision):
    """d(f . site) / d(x_m) by central differences in fp80, h = 1e-6 nm: truncation h^2 x the third derivative (a few 1e-12 relative
    for a frame 0.1 nm across, 1e-10 with the out-of-plane weight 6.4 / nm), rounding 1e-19 / 1e-6."""
    _, kinds, atoms, params = site_system()
    st = state(precision)
    L = np.longdouble
    x, f, p = st["x"].astype(L), st["f"].astype(L), params.astype(L)
    shares = results(precision, L)[1]
    h = L(1e-6)
    worst = 0.0
    for kind in (TWO, THREE, PLANE, LOCAL):
        m = np.flatnonzero(kinds == kind)
        par = [x[atoms[m, 1 + r]] for r in range(3)]
        fs = f[atoms[m, 0]]
        for r in range(2 if kind == TWO else 3):
            for j in range(3):
                up, dn = [q.copy() for q in par], [q.copy() for q in par]
                up[r][:, j] += h; dn[r][:, j] -= h
                e = ((placement(kind, *up, p[m]) - placement(kind, *dn, p[m])) * fs).sum(1) / (2 * h)
                err = np.abs(e - shares[m, r, j]) / np.abs(shares[m]).max(axis=(1, 2))
                worst = max(worst, float(err.max()))
    print(f"transposes against central differences, {precision}: {worst:.2e}")
    assert worst <= 1e-8


@pytest.mark.parametrize("precision", PRECISIONS)
def test_shares_add_up_to_the_force_and_to_its_torque(precision):
    """For weights that sum to 1 (every site of the table) a placement moves with its parents as a rigid body does: the shares carry
    the site's force and its torque about the origin.  In fp80 (2^-64 a rounding, some tens of them: 64 x 2^-64).  An out-of-plane
    site has no such weights (f1 = f - f2 - f3); the others' are fp64 numbers that sum to 1 within a few 2^-53 -- the table test
    asks for 1e-15 -- and miss the invariants by that much: 2^-49 for them."""
    _, kinds, atoms, params = site_system()
    st = state(precision)
    L = np.longdouble
    sites, shares = results(precision, L)
    x, f = st["x"].astype(L), st["f"].astype(L)[atoms[:, 0]]
    tot = shares.sum(1)
    torque = sum(_cross(x[atoms[:, 1 + r]], shares[:, r]) for r in range(3))            # (a two-particle site: a zero share times whatever slot -1 reads)
    scale_f = np.abs(f).max(1)
    scale_t = np.abs(x).max() * scale_f
    plane = kinds == PLANE
    ef = np.abs(tot - f).max(1) / scale_f
    et = np.abs(torque - _cross(sites, f)).max(1) / scale_t
    print(f"sum of shares {precision}: out of plane force {float(ef[plane].max()):.2e} torque {float(et[plane].max()):.2e}; the others {float(ef[~plane].max()):.2e} {float(et[~plane].max()):.2e}")
    assert ef[plane].max() <= 64 * 2.0 ** -64 and et[plane].max() <= 64 * 2.0 ** -64
    assert ef[~plane].max() <= 2.0 ** -49 and et[~plane].max() <= 2.0 ** -49


def test_the_margin_between_twin_and_reference():
    """MEASURED_MARGIN of the module docstring, measured: it must cover the figure, and not by more than a quarter."""
    _, kinds, atoms, params = site_system()
    hard = (kinds == PLANE) | (kinds == LOCAL)
    worst = {"placement": 0.0, "shares": 0.0}
    for precision in PRECISIONS:
        ref, twin = results(precision, np.longdouble), results(precision, np.float64)
        d = np.abs(twin[0].astype(np.longdouble) - ref[0])[hard].max(1) / np.abs(ref[0])[hard].max(1)
        worst["placement"] = max(worst["placement"], float(d.max()))
        d = np.abs(twin[1].astype(np.longdouble) - ref[1])[hard].max(axis=(1, 2)) / np.abs(ref[1])[hard].max(axis=(1, 2))
        worst["shares"] = max(worst["shares"], float(d.max()))
        easy = ~hard                                                                     # the averages: a product per parent, at most two sums
        assert (np.abs(twin[0].astype(np.longdouble) - ref[0])[easy].max(1) / np.abs(ref[0])[easy].max(1)).max() <= 4 * 2.0 ** -53
    figure = max(worst.values())
    print(f"fp64 twin against the fp80 reference: placement {worst['placement']:.3e} shares {worst['shares']:.3e} of the site's largest component; "
          f"MEASURED_MARGIN {MEASURED_MARGIN:.2e}, the GPU gate {GATE:.2e}")
    assert 0.75 * MEASURED_MARGIN <= figure <= MEASURED_MARGIN


# ---------------------------------------------------------------------------
# tgnh_set_virtual_sites on a host-only handle
# ---------------------------------------------------------------------------
def host(s):
    return HostTopology(s, integrator())


def refused(top, kinds, atoms, params, status, match):
    before = top.num_virtual_sites
    with pytest.raises(TgnhError, match=match) as e:
        top.set_virtual_sites(kinds, atoms, params)
    assert e.value.status == status
    assert top.num_virtual_sites == before                                              # a refused table changes nothing


def test_accepted_tables_and_the_count():
    s, kinds, atoms, params = site_system()
    top = host(s)
    assert top.num_virtual_sites == 0
    top.set_virtual_sites(kinds, atoms, params)
    assert top.num_virtual_sites == len(kinds) == 515
    top.set_virtual_sites(kinds[:7], atoms[:7], params[:7])                             # a second table replaces the first
    assert top.num_virtual_sites == 7
    top.set_virtual_sites(np.zeros(0, np.int32), np.zeros((0, 4), np.int32), np.zeros((0, 12)))      # n = 0 clears it
    assert top.num_virtual_sites == 0
    assert top.lib.tgnh_set_virtual_sites(top.h, 0, None, None, None) == _lib.TGNH_OK
    # a two-particle site's p3 is not looked at, as long as it is a slot or -1; parameters a kind does not read may be anything
    k2 = np.flatnonzero(kinds == TWO)[:1]
    a2, p2 = atoms[k2].copy(), params[k2].copy()
    a2[0, 3] = a2[0, 1]
    p2[0, 2:] = np.nan
    top.set_virtual_sites(kinds[k2], a2, p2)
    assert top.num_virtual_sites == 1
    # the launching calls on a host-only handle
    assert top.lib.tgnh_compute_virtual_sites(top.h, None) == _lib.ERR_STATE
    assert top.lib.tgnh_distribute_virtual_site_forces(top.h, None, None) == _lib.ERR_STATE
    top.close()


def test_refusals():
    s, kinds, atoms, params = site_system()
    n = s.num_particles
    order = np.argsort(atoms[:, 0])[:10]                         # the first two rounds: slots 0..27
    k, a, p = kinds[order].copy(), atoms[order].copy(), params[order].copy()
    assert list(k) == [PLANE, PLANE, LOCAL, TWO, THREE, PLANE, PLANE, LOCAL, TWO, THREE] and list(a[4]) == [10, 11, 12, 13]
    top = host(s)
    lib = top.lib
    i32, f64 = lambda v: v.ctypes.data_as(_lib.c_i32p), lambda v: v.ctypes.data_as(_lib.c_f64p)
    assert lib.tgnh_set_virtual_sites(top.h, -1, i32(k), i32(a), f64(p)) == _lib.ERR_ARG
    assert lib.tgnh_set_virtual_sites(top.h, 1, None, i32(a), f64(p)) == _lib.ERR_ARG
    assert lib.tgnh_set_virtual_sites(top.h, 1, i32(k), None, f64(p)) == _lib.ERR_ARG
    assert lib.tgnh_set_virtual_sites(top.h, 1, i32(k), i32(a), None) == _lib.ERR_ARG
    assert lib.tgnh_set_virtual_sites(None, 0, None, None, None) == _lib.ERR_ARG
    assert lib.tgnh_get_num_virtual_sites(top.h, None) == _lib.ERR_ARG

    def with_(ki=None, ai=None, pi=None):
        k2, a2, p2 = k.copy(), a.copy(), p.copy()
        if ki is not None:
            k2[ki[0]] = ki[1]
        if ai is not None:
            a2[ai[0], ai[1]] = ai[2]
        if pi is not None:
            p2[pi[0], pi[1]] = pi[2]
        return k2, a2, p2
    for trial in (0, 1):                                         # on an empty table, then on one in force
        refused(top, *with_(ki=(1, 4)), _lib.ERR_ARG, "site 1: unknown kind 4")
        refused(top, *with_(ki=(1, -1)), _lib.ERR_ARG, "site 1: unknown kind -1")
        refused(top, *with_(ai=(2, 2, n)), _lib.ERR_ARG, "site 2: index %d out of range" % n)
        refused(top, *with_(ai=(2, 0, -1)), _lib.ERR_ARG, "site 2: index -1 out of range")
        refused(top, *with_(ai=(3, 3, -2)), _lib.ERR_ARG, "site 3: index -2 out of range")
        refused(top, *with_(ai=(1, 0, 3)), _lib.ERR_ARG, "site 1: slot 3 is listed as a site twice")
        refused(top, *with_(ai=(0, 2, 0)), _lib.ERR_ARG, "site 0 lists parent 0 twice")
        refused(top, *with_(ai=(3, 2, 5)), _lib.ERR_ARG, "site 3 lists parent 5 twice")
        refused(top, *with_(ai=(5, 3, 3)), _lib.ERR_ARG, "site 5: parent 3 is itself a site")
        refused(top, *with_(ai=(4, 1, 10)), _lib.ERR_ARG, "site 4: parent 10 is itself a site")            # ... its own
        for row in (0, 2, 4):                                    # the three kinds that need three parents
            refused(top, *with_(ai=(row, 3, -1)), _lib.ERR_ARG, "site %d: p3 = -1" % row)
        refused(top, *with_(pi=(3, 1, np.nan)), _lib.ERR_ARG, "site 3: a parameter is not finite")
        refused(top, *with_(pi=(0, 2, np.inf)), _lib.ERR_ARG, "site 0: a parameter is not finite")
        refused(top, *with_(pi=(2, 11, -np.inf)), _lib.ERR_ARG, "site 2: a parameter is not finite")
        refused(top, *with_(pi=(2, 0, p[2, 0] + 2e-6)), _lib.ERR_ARG, "site 2: the origin weights do not sum to 1")
        refused(top, *with_(pi=(2, 4, p[2, 4] - 2e-6)), _lib.ERR_ARG, "site 2: the x or y weights do not sum to 0")
        refused(top, *with_(pi=(7, 8, p[7, 8] + 2e-6)), _lib.ERR_ARG, "site 7: the x or y weights do not sum to 0")
        top.set_virtual_sites(*with_(pi=(2, 0, p[2, 0] + 5e-7)))                                           # inside OpenMM's gate
        # what this stage does not take: a site with a mass, a site in a Drude pair
        # what this stage does not take: a site with a mass (slot 28: the next round's oxygen, nobody's parent in these ten rows)
        refused(top, *with_(ai=(8, 0, 28)), _lib.ERR_UNSUPPORTED, "site 8: slot 28 has a mass")
        assert top.num_virtual_sites == 10
        top.set_virtual_sites(k, a, p)
    top.close()
    # ... and a site that a Drude pair names: SWM4 water, O D H1 H2 M per molecule, (D, O) the pair
    from openmm_drudenose_amd import synth
    top = host(synth.water_box(2)[0])
    w3 = np.array([[0.8, 0.1, 0.1] + [0.0] * 9, [0.8, 0.1, 0.1] + [0.0] * 9])
    refused(top, [THREE, THREE], [[4, 0, 2, 3], [6, 5, 7, 8]], w3, _lib.ERR_UNSUPPORTED, "site 1: slot 6 is a member of a Drude pair")      # the Drude particle
    refused(top, [THREE, THREE], [[0, 5, 2, 3], [9, 5, 7, 8]], w3, _lib.ERR_UNSUPPORTED, "site 0: slot 0 is a member of a Drude pair")      # its parent
    refused(top, [THREE, THREE], [[4, 0, 2, 3], [7, 5, 9, 8]], w3, _lib.ERR_UNSUPPORTED, "site 1: slot 7 has a mass")
    refused(top, [THREE, THREE], [[4, 0, 2, 3], [9, 5, 7, 4]], w3, _lib.ERR_ARG, "site 1: parent 4 is itself a site")                      # (ERR_ARG goes first)
    top.set_virtual_sites([THREE, THREE], [[4, 0, 2, 3], [9, 5, 7, 8]], w3)
    assert top.num_virtual_sites == 2
    top.close()


def test_system_site_table():
    s = site_system()[0]
    t = DrudeSystem(mass=s.mass, pair_drude=s.pair_drude, pair_parent=s.pair_parent, resid=s.resid)
    assert t.site_table_kinds is None
    t.set_site_table([TWO, PLANE], [[4, 0, 1, -1], [3, 0, 1, 2]], [[0.5, 0.5, 0.0], [0.1, 0.2, 0.3]])       # short rows are padded
    assert t.site_table_kinds.dtype == np.int32 and t.site_table_atoms.shape == (2, 4) and t.site_table_params.shape == (2, 12)
    assert np.array_equal(t.site_table_params[1, :4], [0.1, 0.2, 0.3, 0.0])
    top = host(t)
    top.set_virtual_sites(t.site_table_kinds, t.site_table_atoms, t.site_table_params)
    assert top.num_virtual_sites == 2
    with pytest.raises(TgnhError, match="one kind, one row of atoms"):
        top.set_virtual_sites([TWO], t.site_table_atoms, t.site_table_params)
    top.close()
