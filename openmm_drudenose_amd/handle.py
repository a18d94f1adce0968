"""The library handle and everything a host-only handle answers as well as a device context: tgnh_create, the lifetime, and the
tables and queries of include/drude_tgnh.h that need no device -- dof terms, thermostat state, topology, molecules, constraint
clusters, virtual sites, DrudeForce, the periodic box.

`Handle` is the common base of `HostTopology` and of every part `HipContext` is assembled from (context.py).  It declares what
those parts may rely on: `lib`, `h`, `n`, `padded`, `group`, `num_groups`, `_stream()`, `_get()`, `_vec()`, and -- set by the
context's constructor -- `dev`, `torch`, `integrator`.  A new table goes here; its launches go to the feature's module."""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import TgnhError, _check, out, f64, i32
from .synth import KB

_PREC = {"single": _lib.PREC_SINGLE, "mixed": _lib.PREC_MIXED, "double": _lib.PREC_DOUBLE}
_MODE = {"dualNH": _lib.MODE_DUALNH, "TGNH": _lib.MODE_TGNH}

MAX_DIRECT_CONSTRAINTS = 3      # constraints per cluster that tgnh_set_constraint_clusters takes (csrc/tgnh_constraints.h)


def split_clusters(atoms, dist):
    """Constraint clusters in the canonical form ([K,4] slot indices, -1 = unused; [K,6] distances, 0 = none) -> (direct, rest), each
    an (atoms, dist) pair: the clusters of at most three constraints, which the library's direct solver takes
    (tgnh_set_constraint_clusters), and the others, which stay with the harness' iterative SHAKE.  Every cluster lands on exactly
    one side, and each side keeps the order it came in.  Pure numpy: no handle, no device."""
    atoms, dist = i32(atoms, (-1, 4))[0], f64(dist, (-1, 6))[0]
    if len(atoms) != len(dist):
        raise TgnhError(_lib.ERR_ARG, "split_clusters: one row of distances per cluster")
    direct = (dist != 0).sum(1) <= MAX_DIRECT_CONSTRAINTS
    return ((np.ascontiguousarray(atoms[direct]), np.ascontiguousarray(dist[direct])),
            (np.ascontiguousarray(atoms[~direct]), np.ascontiguousarray(dist[~direct])))


def create_handle(lib, system, integrator, group, ngroups, mode, precision, device, flags, kB, padded):
    """tgnh_create from a DrudeSystem + integrator mirror.  device = -1 gives a host-only handle."""
    d = _lib.TgnhDesc(struct_size=C.sizeof(_lib.TgnhDesc))
    d.mode, d.precision, d.flags, d.device = mode, precision, int(flags), device
    d.num_particles, d.padded_num_particles = system.num_particles, padded
    d.num_pairs, d.num_groups, d.num_residues = system.num_pairs, ngroups, system.num_residues
    d.num_constraints, d.has_cm_motion_remover = len(system.constraints), int(system.has_cm_motion_remover)
    group, d.group = i32(group)
    d.mass = system.mass.ctypes.data_as(_lib.c_f64p)
    d.pair_drude, d.pair_parent, d.resid = (a.ctypes.data_as(_lib.c_i32p) for a in (system.pair_drude, system.pair_parent, system.resid))
    if len(system.constraints):
        (ci, d.constraint_i), (cj, d.constraint_j) = i32(system.constraints[:, 0]), i32(system.constraints[:, 1])
    d.kB, d.temperature, d.coupling_time = kB, integrator.getTemperature(), integrator.getCouplingTime()
    d.drude_temperature, d.drude_coupling_time = integrator.getDrudeTemperature(), integrator.getDrudeCouplingTime()
    d.step_size, d.drude_steps_per_real_step = integrator.getStepSize(), integrator.getDrudeStepsPerRealStep()
    d.num_nh_chains, d.max_drude_distance = integrator.getNumNHChains(), integrator.getMaxDrudeDistance()
    d.use_drude_nh_chains, d.use_com_temp_group = integrator.getUseDrudeNHChains(), integrator.getUseCOMTempGroup()
    h = C.c_void_p()
    _check(lib.tgnh_create(C.byref(d), C.byref(h)))
    return h


class Handle:
    """Owns the library handle; the tables and queries shared by device contexts and host-only handles."""

    def _open(self, system, integrator, mode, precision, device, flags, kB):
        """lib, n, padded, group, num_groups and h: the handle on `device` (-1: host-only)"""
        self.lib = _lib.load()
        self.n = system.num_particles
        self.padded = (self.n + 31) // 32 * 32               # OpenMM PADDED_NUM_ATOMS (TileSize 32)
        self.group, self.num_groups = integrator._resolve_groups(self.n)
        self.h = create_handle(self.lib, system, integrator, self.group, self.num_groups, _MODE[mode], _PREC[precision], device, flags,
                               kB, self.padded)

    def close(self):
        if getattr(self, "h", None):
            self.lib.tgnh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        return None

    def _get(self, fn, types=C.c_int, *args, stream=False, check=True):
        """fn(h, *args[, stream], &v...) -> v (see _abi.out)"""
        return out(fn, types, self.h, *args, *([self._stream()] if stream else []), check=check)

    def _vec(self, fn, n, *args):
        """fn(h, *args, stream, double[n]) -> the array"""
        a, p = f64(np.zeros(n))
        _check(fn(self.h, *args, self._stream(), p))
        return a

    # ---- path, degrees of freedom, thermostat state, topology (tgnh_queries) ----
    def step_path(self):
        """('tiled', '') or ('gather', why): the reference's own un-fused kernels by global index, for what the tiles cannot hold"""
        g, why = self._get(self.lib.tgnh_get_step_path, (C.c_int, C.c_char_p))
        return ("tiled", "gather", "gather")[g], (why or b"").decode()

    def local_dof_terms(self):
        a, p = f64(np.zeros(self._get(self.lib.tgnh_get_local_dof_terms, C.c_int, None)))
        self._get(self.lib.tgnh_get_local_dof_terms, C.c_int, p)
        return a

    def set_global_dof_terms(self, total):
        total, p = f64(total)
        _check(self.lib.tgnh_set_global_dof_terms(self.h, p, len(total)))

    def num_thermostats(self): return self._get(self.lib.tgnh_get_num_thermostats)

    def dof(self):
        n = self.num_thermostats()
        (dof, pd), (nkt, pn) = f64(np.zeros(n)), f64(np.zeros(n))
        _check(self.lib.tgnh_get_dof(self.h, pd, pn))
        return dof, nkt

    def thermostat_state(self, which):
        return self._vec(self.lib.tgnh_get_thermostat_state, self._get(self.lib.tgnh_get_thermostat_len, C.c_int, which), which)

    def set_thermostat_state(self, which, arr):
        _check(self.lib.tgnh_set_thermostat_state(self.h, which, self._stream(), f64(arr)[1]))

    def topology(self, which):
        a, p = i32(np.zeros(self._get(self.lib.tgnh_get_topology_len, C.c_int, which), np.int32))
        _check(self.lib.tgnh_get_topology(self.h, which, p))
        return a

    # ---- the molecule table (include/drude_tgnh.h: tgnh_set_molecules, ...): what scale_positions moves rigidly ----
    def set_molecules(self, labels=None):
        """tgnh_set_molecules: one int32 label per slot, equal labels one molecule (consecutive or not); None: the default, the
        system's residues.  A Drude pair split between two molecules is refused."""
        _check(self.lib.tgnh_set_molecules(self.h, None if labels is None else
                                           i32(labels, (self.n,), "set_molecules", "one label per particle slot")[1]))

    def num_molecules(self):
        """tgnh_get_num_molecules: M, the number of molecules of the table in force (a barostat's acceptance rule needs it)."""
        return self._get(self.lib.tgnh_get_num_molecules)

    def molecules(self):
        """tgnh_get_molecules: the labels renumbered 0..M-1 in order of first appearance."""
        a, p = i32(np.zeros(self.n, np.int32))
        _check(self.lib.tgnh_get_molecules(self.h, p))
        return a

    # ---- the direct constraint solver's cluster table (include/drude_tgnh.h: tgnh_set_constraint_clusters) ----
    def set_constraint_clusters(self, atoms, dist):
        """tgnh_set_constraint_clusters: clusters of one to three constraints in the canonical form; an empty table clears it.  The
        checks run on a host-only handle too."""
        (atoms, pa), (dist, pd) = i32(atoms, (-1, 4)), f64(dist, (-1, 6))
        if len(atoms) != len(dist):
            raise TgnhError(_lib.ERR_ARG, "set_constraint_clusters: one row of distances per cluster")
        _check(self.lib.tgnh_set_constraint_clusters(self.h, len(atoms), pa, pd))

    def num_constraint_clusters(self):
        """tgnh_get_num_constraint_clusters: the clusters of the direct solver's table"""
        return self._get(self.lib.tgnh_get_num_constraint_clusters)

    # ---- the library's own virtual-site table (include/drude_tgnh.h: tgnh_set_virtual_sites) ----
    def set_virtual_sites(self, kinds, atoms, params):
        """tgnh_set_virtual_sites: kinds [S] (_lib.SITE_*), atoms [S,4] = (site, p1, p2, p3) with p3 = -1 for a two-particle site,
        params [S,12]; an empty table clears it.  The checks run on a host-only handle too."""
        (kinds, pk), (atoms, pa), (params, pp) = i32(kinds, (-1,)), i32(atoms, (-1, 4)), f64(params, (-1, _lib.SITE_PARAMS))
        if not len(kinds) == len(atoms) == len(params):
            raise TgnhError(_lib.ERR_ARG, "set_virtual_sites: one kind, one row of atoms and one row of twelve parameters per site")
        _check(self.lib.tgnh_set_virtual_sites(self.h, len(kinds), pk, pa, pp))

    @property
    def num_virtual_sites(self):
        """tgnh_get_num_virtual_sites: the sites of the library's table"""
        return self._get(self.lib.tgnh_get_num_virtual_sites)

    # ---- the library's own DrudeForce table (include/drude_tgnh.h: tgnh_set_drude_force) ----
    def set_drude_force(self, force):
        """tgnh_set_drude_force: a forces.DrudeForce, or its four tables (particles [n,5], params [n,4], screened [m,2], thole [m]);
        row k names the system's pair k; None or an empty table clears it.  The checks run on a host-only handle too."""
        if force is None:
            return _check(self.lib.tgnh_set_drude_force(self.h, 0, None, None, 0, None, None))
        particles, params, screened, thole = force.tables() if hasattr(force, "tables") else force
        (particles, pp), (params, pq) = i32(particles, (-1, 5)), f64(params, (-1, 4))
        (screened, ps), (thole, pt) = i32(screened, (-1, 2)), f64(thole, (-1,))
        if len(particles) != len(params) or len(screened) != len(thole):
            raise TgnhError(_lib.ERR_ARG, "set_drude_force: one row of four parameters per row of particles, one thole per screened pair")
        _check(self.lib.tgnh_set_drude_force(self.h, len(particles), pp, pq, len(screened), ps, pt))

    @property
    def num_drude_force_terms(self):
        """tgnh_get_num_drude_force_terms: (rows, screened pairs) of the table in force"""
        return self._get(self.lib.tgnh_get_num_drude_force_terms, (C.c_int, C.c_int))

    # ---- the periodic box and the size of a frame (include/drude_tgnh.h: tgnh_set_periodic_box, tgnh_get_frame_count) ----
    def setPeriodicBoxVectors(self, a, b, c):
        """tgnh_set_periodic_box: the three box vectors (nm) in OpenMM's reduced form -- a = (ax, 0, 0), b = (bx, by, 0),
        c = (cx, cy, cz), ax, by, cz > 0, ax >= 2 |bx|, ax >= 2 |cx|, by >= 2 |cy| --; anything else is refused and the box in force
        stays.  Kept on the host: wrap_molecules() and frame(wrap=True) take it along by value."""
        v = [f64(x, (3,), "setPeriodicBoxVectors", "three vectors of three components")[1] for x in (a, b, c)]
        _check(self.lib.tgnh_set_periodic_box(self.h, *v))

    def getPeriodicBoxVectors(self):
        """tgnh_get_periodic_box: the box vectors as they were set, a [3, 3] array of rows a, b, c (nm); None before the first set."""
        box = np.zeros((3, 3))
        rc = self.lib.tgnh_get_periodic_box(self.h, *[box[k].ctypes.data_as(_lib.c_f64p) for k in range(3)])
        if rc == _lib.ERR_STATE:
            return None
        _check(rc)
        return box

    def frame_count(self, skip_drude=False):
        """tgnh_get_frame_count: the atoms of a frame -- every slot, or every slot that is no Drude particle."""
        return self._get(self.lib.tgnh_get_frame_count, C.c_int64, _lib.FRAME_SKIP_DRUDE if skip_drude else 0)


class HostTopology(Handle):
    """Host-only handle (device -1): the library's topology / tile / dof logic without a GPU.  Used by the CPU
    tests; it cannot launch anything."""

    def __init__(self, system, integrator, mode="TGNH", precision="mixed", flags=0, kB=KB):
        self._open(system, integrator, mode, precision, -1, flags, kB)
