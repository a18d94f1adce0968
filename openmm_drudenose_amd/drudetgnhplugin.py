"""Host-side mirror of the reference's Python surface over the HIP C ABI.

`DrudeTGNHIntegrator` keeps the method names, argument meaning, defaults and error
behaviour of the SWIG class (python/drudetgnhplugin.i:60-92 of scychon/openmm_drudeNose,
C++ side openmmapi/src/DrudeTGNHIntegrator.cpp).  OpenMM is not available here, so
`HipContext` stands where OpenMM's Context + HIP platform would: it owns the device
arrays in OpenMM's layouts (posq real4, velm mixed4 with w = 1/m, force int64 x 2^32 in
three planes, posqCorrection in mixed precision) and drives the C ABI.  torch is used
for device memory, streams and torch.distributed only.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (MODE_DUALNH, MODE_TGNH, PREC_SINGLE, PREC_MIXED, PREC_DOUBLE,  # noqa: F401
                   FLAG_DEFER_SCALE, FLAG_RESIDENT_STEP, FLAG_WAVE_TILES, FLAG_TRUST_STATE_CHANGED, FLAG_GATHER)
from .synth import KB

_PREC = {"single": PREC_SINGLE, "mixed": PREC_MIXED, "double": PREC_DOUBLE}
_MODE = {"dualNH": MODE_DUALNH, "TGNH": MODE_TGNH}


class TgnhError(RuntimeError):
    """Stands for OpenMMException; .status is the C-ABI status code."""

    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


def _check(rc):
    if rc != _lib.TGNH_OK:
        raise TgnhError(rc, _lib.load().tgnh_last_error().decode())


class DrudeTGNHIntegrator:
    """Same constructor and methods as the reference's SWIG class (drudetgnhplugin.i:60-92).
    Note the Python default useDrudeNHChains=True (the C++ default is false,
    DrudeTGNHIntegrator.h:71)."""

    def __init__(self, temperature, couplingTime, drudeTemperature, drudeCouplingTime, stepSize,
                 drudeStepsPerRealStep=20, numNHChains=1, useDrudeNHChains=True, useCOMTempGroup=True):
        self._temperature = float(temperature)
        self._couplingTime = float(couplingTime)
        self._drudeTemperature = float(drudeTemperature)
        self._drudeCouplingTime = float(drudeCouplingTime)
        self._maxDrudeDistance = 0.0
        self._stepSize = float(stepSize)
        self._drudeSteps = int(drudeStepsPerRealStep)
        self._numNHChains = int(numNHChains)
        self._useDrudeNHChains = bool(useDrudeNHChains)
        self._useCOMTempGroup = bool(useCOMTempGroup)
        self._constraintTolerance = 1e-5                     # DrudeTGNHIntegrator.cpp:58
        self._tempGroups = []
        self._particleTempGroup = []
        self._context = None

    # --- scalar properties (DrudeTGNHIntegrator.h:77-211) ---
    def getTemperature(self): return self._temperature

    def setTemperature(self, temp):
        self._set_bath("_temperature", temp)
    def getCouplingTime(self): return self._couplingTime
    def setCouplingTime(self, tau): self._couplingTime = float(tau)
    def getDrudeTemperature(self): return self._drudeTemperature

    def setDrudeTemperature(self, temp):
        self._set_bath("_drudeTemperature", temp)

    def _set_bath(self, name, temp):
        """A bound integrator retargets its handle (tgnh_set_temperatures); where the handle refuses -- between the steps of a
        deferred sequence, or a value that is no temperature -- the integrator keeps the value the handle runs at."""
        old = getattr(self, name)
        setattr(self, name, float(temp))
        if self._context is not None:
            try:
                self._context._push_scalars()
            except TgnhError:
                setattr(self, name, old)
                raise

    def getDrudeCouplingTime(self): return self._drudeCouplingTime
    def setDrudeCouplingTime(self, tau): self._drudeCouplingTime = float(tau)
    def getMaxDrudeDistance(self): return self._maxDrudeDistance

    def setMaxDrudeDistance(self, distance):
        if distance < 0:                                     # DrudeTGNHIntegrator.cpp:97-100
            raise TgnhError(_lib.ERR_ARG, "setMaxDrudeDistance: Distance cannot be negative")
        self._maxDrudeDistance = float(distance)
        if self._context is not None:
            self._context._push_scalars()

    def getStepSize(self): return self._stepSize

    def setStepSize(self, dt):
        self._stepSize = float(dt)
        if self._context is not None:
            self._context._push_scalars()

    def getConstraintTolerance(self): return self._constraintTolerance
    def setConstraintTolerance(self, tol): self._constraintTolerance = float(tol)
    def getDrudeStepsPerRealStep(self): return self._drudeSteps

    def setDrudeStepsPerRealStep(self, drudeSteps):
        self._drudeSteps = int(drudeSteps)
        if self._context is not None:
            self._context._push_scalars()

    def getNumNHChains(self): return self._numNHChains
    def setNumNHChains(self, numChains): self._numNHChains = int(numChains)
    def getUseDrudeNHChains(self): return int(self._useDrudeNHChains)
    def setUseDrudeNHChains(self, use): self._useDrudeNHChains = bool(use)
    def getUseCOMTempGroup(self): return int(self._useCOMTempGroup)
    def setUseCOMTempGroup(self, use): self._useCOMTempGroup = bool(use)

    # --- temperature groups (DrudeTGNHIntegrator.cpp:61-86) ---
    def getNumTempGroups(self): return len(self._tempGroups)

    def addTempGroup(self):
        self._tempGroups.append(len(self._tempGroups))
        return len(self._tempGroups) - 1

    def addParticleTempGroup(self, tempGroup):
        if not 0 <= tempGroup < len(self._tempGroups):       # ASSERT_VALID_INDEX
            raise TgnhError(_lib.ERR_ARG, "Index out of range")
        if not isinstance(self._particleTempGroup, list):    # (the defaults of _resolve_groups are an array)
            self._particleTempGroup = [int(x) for x in self._particleTempGroup]
        self._particleTempGroup.append(int(tempGroup))
        return len(self._particleTempGroup) - 1

    def setParticleTempGroup(self, particle, tempGroup):
        if not 0 <= particle < len(self._particleTempGroup) or not 0 <= tempGroup < len(self._tempGroups):
            raise TgnhError(_lib.ERR_ARG, "Index out of range")
        self._particleTempGroup[particle] = int(tempGroup)

    def getParticleTempGroup(self, particle):
        if not 0 <= particle < len(self._particleTempGroup):
            raise TgnhError(_lib.ERR_ARG, "Index out of range")
        return int(self._particleTempGroup[particle])

    # --- stepping (DrudeTGNHIntegrator.cpp:182-194) ---
    def step(self, steps):
        if self._context is None:
            raise TgnhError(_lib.ERR_STATE, "This Integrator is not bound to a context!")
        self._context.step(steps)

    def computeKineticEnergy(self):
        return self._context.kinetic_energy()

    def _resolve_groups(self, num_particles):
        """DrudeTGNHIntegrator.cpp:126-134: default everything to one group; else the count must match."""
        if len(self._particleTempGroup) == 0:
            if len(self._tempGroups) == 0:
                self._tempGroups.append(0)
            # (an array: a Python list of millions of ints is walked by every full pass of the garbage collector)
            self._particleTempGroup = np.zeros(num_particles, np.int32)
        elif len(self._particleTempGroup) != num_particles:
            raise TgnhError(_lib.ERR_ARG, "Number of particles assigned with temperature groups does not match the number of system particles")
        return np.asarray(self._particleTempGroup, np.int32), len(self._tempGroups)


MAX_DIRECT_CONSTRAINTS = 3      # constraints per cluster that tgnh_set_constraint_clusters takes (csrc/tgnh_constraints.h)


def split_clusters(atoms, dist):
    """Constraint clusters in the canonical form ([K,4] slot indices, -1 = unused; [K,6] distances, 0 = none) -> (direct, rest), each
    an (atoms, dist) pair: the clusters of at most three constraints, which the library's direct solver takes
    (tgnh_set_constraint_clusters), and the others, which stay with the harness' iterative SHAKE.  Every cluster lands on exactly
    one side, and each side keeps the order it came in.  Pure numpy: no handle, no device."""
    atoms = np.ascontiguousarray(atoms, np.int32).reshape(-1, 4)
    dist = np.ascontiguousarray(dist, np.float64).reshape(-1, 6)
    if len(atoms) != len(dist):
        raise TgnhError(_lib.ERR_ARG, "split_clusters: one row of distances per cluster")
    direct = (dist != 0).sum(1) <= MAX_DIRECT_CONSTRAINTS
    return ((np.ascontiguousarray(atoms[direct]), np.ascontiguousarray(dist[direct])),
            (np.ascontiguousarray(atoms[~direct]), np.ascontiguousarray(dist[~direct])))


def create_handle(lib, system, integrator, group, ngroups, mode, precision, device, flags, kB, padded):
    """tgnh_create from a DrudeSystem + integrator mirror.  device = -1 gives a host-only handle."""
    n = system.num_particles
    d = _lib.TgnhDesc()
    d.struct_size = C.sizeof(_lib.TgnhDesc)
    d.mode, d.precision, d.flags, d.device = mode, precision, int(flags), device
    d.num_particles, d.padded_num_particles = n, padded
    d.num_pairs, d.num_groups, d.num_residues = system.num_pairs, ngroups, system.num_residues
    d.num_constraints = len(system.constraints)
    d.has_cm_motion_remover = int(system.has_cm_motion_remover)
    group = np.ascontiguousarray(group, np.int32)
    ci = np.ascontiguousarray(system.constraints[:, 0]) if len(system.constraints) else None
    cj = np.ascontiguousarray(system.constraints[:, 1]) if len(system.constraints) else None
    d.mass = system.mass.ctypes.data_as(_lib.c_f64p)
    d.pair_drude = system.pair_drude.ctypes.data_as(_lib.c_i32p)
    d.pair_parent = system.pair_parent.ctypes.data_as(_lib.c_i32p)
    d.group = group.ctypes.data_as(_lib.c_i32p)
    d.resid = system.resid.ctypes.data_as(_lib.c_i32p)
    if ci is not None:
        d.constraint_i = ci.ctypes.data_as(_lib.c_i32p)
        d.constraint_j = cj.ctypes.data_as(_lib.c_i32p)
    d.kB = kB
    d.temperature, d.coupling_time = integrator.getTemperature(), integrator.getCouplingTime()
    d.drude_temperature, d.drude_coupling_time = integrator.getDrudeTemperature(), integrator.getDrudeCouplingTime()
    d.step_size = integrator.getStepSize()
    d.drude_steps_per_real_step = integrator.getDrudeStepsPerRealStep()
    d.num_nh_chains = integrator.getNumNHChains()
    d.use_drude_nh_chains = integrator.getUseDrudeNHChains()
    d.use_com_temp_group = integrator.getUseCOMTempGroup()
    d.max_drude_distance = integrator.getMaxDrudeDistance()
    h = C.c_void_p()
    _check(lib.tgnh_create(C.byref(d), C.byref(h)))
    return h


class _HandleQueries:
    """Queries shared by device contexts and host-only handles."""

    def _stream(self):
        return None

    def step_path(self):
        """('tiled', '') or ('gather', why): the reference's own un-fused kernels by global index, for what the tiles cannot hold"""
        g, why = C.c_int(), C.c_char_p()
        _check(self.lib.tgnh_get_step_path(self.h, C.byref(g), C.byref(why)))
        return ("tiled", "gather", "gather")[g.value], (why.value or b"").decode()

    def local_dof_terms(self):
        n = C.c_int()
        _check(self.lib.tgnh_get_local_dof_terms(self.h, None, C.byref(n)))
        out = np.zeros(n.value)
        _check(self.lib.tgnh_get_local_dof_terms(self.h, out.ctypes.data_as(_lib.c_f64p), C.byref(n)))
        return out

    def set_global_dof_terms(self, total):
        total = np.ascontiguousarray(total, np.float64)
        _check(self.lib.tgnh_set_global_dof_terms(self.h, total.ctypes.data_as(_lib.c_f64p), len(total)))

    def num_thermostats(self):
        n = C.c_int()
        _check(self.lib.tgnh_get_num_thermostats(self.h, C.byref(n)))
        return n.value

    def dof(self):
        n = self.num_thermostats()
        dof, nkt = np.zeros(n), np.zeros(n)
        _check(self.lib.tgnh_get_dof(self.h, dof.ctypes.data_as(_lib.c_f64p), nkt.ctypes.data_as(_lib.c_f64p)))
        return dof, nkt

    def thermostat_state(self, which):
        n = C.c_int()
        _check(self.lib.tgnh_get_thermostat_len(self.h, which, C.byref(n)))
        out = np.zeros(n.value)
        _check(self.lib.tgnh_get_thermostat_state(self.h, which, self._stream(), out.ctypes.data_as(_lib.c_f64p)))
        return out

    def set_thermostat_state(self, which, arr):
        arr = np.ascontiguousarray(arr, np.float64)
        _check(self.lib.tgnh_set_thermostat_state(self.h, which, self._stream(), arr.ctypes.data_as(_lib.c_f64p)))

    def topology(self, which):
        n = C.c_int()
        _check(self.lib.tgnh_get_topology_len(self.h, which, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        _check(self.lib.tgnh_get_topology(self.h, which, out.ctypes.data_as(_lib.c_i32p)))
        return out


    # ---- the molecule table (include/drude_tgnh.h: tgnh_set_molecules, ...): what scale_positions moves rigidly ----
    def set_molecules(self, labels=None):
        """tgnh_set_molecules: one int32 label per slot, equal labels one molecule (consecutive or not); None: the default, the
        system's residues.  A Drude pair split between two molecules is refused."""
        if labels is None:
            _check(self.lib.tgnh_set_molecules(self.h, None))
            return
        lab = np.ascontiguousarray(labels, np.int32)
        n = self.n
        if lab.shape != (n,):
            raise TgnhError(_lib.ERR_ARG, "set_molecules: one label per particle slot")
        _check(self.lib.tgnh_set_molecules(self.h, lab.ctypes.data_as(_lib.c_i32p)))

    def num_molecules(self):
        """tgnh_get_num_molecules: M, the number of molecules of the table in force (a barostat's acceptance rule needs it)."""
        n = C.c_int()
        _check(self.lib.tgnh_get_num_molecules(self.h, C.byref(n)))
        return n.value

    def molecules(self):
        """tgnh_get_molecules: the labels renumbered 0..M-1 in order of first appearance."""
        out = np.zeros(self.n, np.int32)
        _check(self.lib.tgnh_get_molecules(self.h, out.ctypes.data_as(_lib.c_i32p)))
        return out

    # ---- the direct constraint solver's cluster table (include/drude_tgnh.h: tgnh_set_constraint_clusters) ----
    def set_constraint_clusters(self, atoms, dist):
        """tgnh_set_constraint_clusters: clusters of one to three constraints in the canonical form; an empty table clears it.  The
        checks run on a host-only handle too."""
        atoms = np.ascontiguousarray(atoms, np.int32).reshape(-1, 4)
        dist = np.ascontiguousarray(dist, np.float64).reshape(-1, 6)
        if len(atoms) != len(dist):
            raise TgnhError(_lib.ERR_ARG, "set_constraint_clusters: one row of distances per cluster")
        _check(self.lib.tgnh_set_constraint_clusters(self.h, len(atoms), atoms.ctypes.data_as(_lib.c_i32p), dist.ctypes.data_as(_lib.c_f64p)))

    def num_constraint_clusters(self):
        """tgnh_get_num_constraint_clusters: the clusters of the direct solver's table"""
        n = C.c_int()
        _check(self.lib.tgnh_get_num_constraint_clusters(self.h, C.byref(n)))
        return n.value

    # ---- the library's own virtual-site table (include/drude_tgnh.h: tgnh_set_virtual_sites) ----
    def set_virtual_sites(self, kinds, atoms, params):
        """tgnh_set_virtual_sites: kinds [S] (_lib.SITE_*), atoms [S,4] = (site, p1, p2, p3) with p3 = -1 for a two-particle site,
        params [S,12]; an empty table clears it.  The checks run on a host-only handle too."""
        kinds = np.ascontiguousarray(kinds, np.int32).reshape(-1)
        atoms = np.ascontiguousarray(atoms, np.int32).reshape(-1, 4)
        params = np.ascontiguousarray(params, np.float64).reshape(-1, _lib.SITE_PARAMS)
        if not len(kinds) == len(atoms) == len(params):
            raise TgnhError(_lib.ERR_ARG, "set_virtual_sites: one kind, one row of atoms and one row of twelve parameters per site")
        _check(self.lib.tgnh_set_virtual_sites(self.h, len(kinds), kinds.ctypes.data_as(_lib.c_i32p), atoms.ctypes.data_as(_lib.c_i32p),
                                               params.ctypes.data_as(_lib.c_f64p)))

    @property
    def num_virtual_sites(self):
        """tgnh_get_num_virtual_sites: the sites of the library's table"""
        n = C.c_int()
        _check(self.lib.tgnh_get_num_virtual_sites(self.h, C.byref(n)))
        return n.value

    # ---- the library's own DrudeForce table (include/drude_tgnh.h: tgnh_set_drude_force) ----
    def set_drude_force(self, force):
        """tgnh_set_drude_force: a forces.DrudeForce, or its four tables (particles [n,5], params [n,4], screened [m,2], thole [m]);
        row k names the system's pair k; None or an empty table clears it.  The checks run on a host-only handle too."""
        if force is None:
            _check(self.lib.tgnh_set_drude_force(self.h, 0, None, None, 0, None, None))
            return
        particles, params, screened, thole = force.tables() if hasattr(force, "tables") else force
        particles = np.ascontiguousarray(particles, np.int32).reshape(-1, 5)
        params = np.ascontiguousarray(params, np.float64).reshape(-1, 4)
        screened = np.ascontiguousarray(screened, np.int32).reshape(-1, 2)
        thole = np.ascontiguousarray(thole, np.float64).reshape(-1)
        if len(particles) != len(params) or len(screened) != len(thole):
            raise TgnhError(_lib.ERR_ARG, "set_drude_force: one row of four parameters per row of particles, one thole per screened pair")
        _check(self.lib.tgnh_set_drude_force(self.h, len(particles), particles.ctypes.data_as(_lib.c_i32p), params.ctypes.data_as(_lib.c_f64p),
                                             len(screened), screened.ctypes.data_as(_lib.c_i32p), thole.ctypes.data_as(_lib.c_f64p)))

    @property
    def num_drude_force_terms(self):
        """tgnh_get_num_drude_force_terms: (rows, screened pairs) of the table in force"""
        n, m = C.c_int(), C.c_int()
        _check(self.lib.tgnh_get_num_drude_force_terms(self.h, C.byref(n), C.byref(m)))
        return n.value, m.value

    # ---- the periodic box and the size of a frame (include/drude_tgnh.h: tgnh_set_periodic_box, tgnh_get_frame_count) ----
    def setPeriodicBoxVectors(self, a, b, c):
        """tgnh_set_periodic_box: the three box vectors (nm) in OpenMM's reduced form -- a = (ax, 0, 0), b = (bx, by, 0),
        c = (cx, cy, cz), ax, by, cz > 0, ax >= 2 |bx|, ax >= 2 |cx|, by >= 2 |cy| --; anything else is refused and the box in force
        stays.  Kept on the host: wrap_molecules() and frame(wrap=True) take it along by value."""
        v = [np.ascontiguousarray(x, np.float64) for x in (a, b, c)]
        if any(x.shape != (3,) for x in v):
            raise TgnhError(_lib.ERR_ARG, "setPeriodicBoxVectors: three vectors of three components")
        _check(self.lib.tgnh_set_periodic_box(self.h, *[x.ctypes.data_as(_lib.c_f64p) for x in v]))

    def getPeriodicBoxVectors(self):
        """tgnh_get_periodic_box: the box vectors as they were set, a [3, 3] array of rows a, b, c (nm); None before the first set."""
        out = np.zeros((3, 3))
        rc = self.lib.tgnh_get_periodic_box(self.h, *[out[k].ctypes.data_as(_lib.c_f64p) for k in range(3)])
        if rc == _lib.ERR_STATE:
            return None
        _check(rc)
        return out

    def frame_count(self, skip_drude=False):
        """tgnh_get_frame_count: the atoms of a frame -- every slot, or every slot that is no Drude particle."""
        n = C.c_int64()
        _check(self.lib.tgnh_get_frame_count(self.h, _lib.FRAME_SKIP_DRUDE if skip_drude else 0, C.byref(n)))
        return n.value


class HostTopology(_HandleQueries):
    """Host-only handle (device -1): the library's topology / tile / dof logic without a GPU.  Used by the CPU
    tests; it cannot launch anything."""

    def __init__(self, system, integrator, mode="TGNH", precision="mixed", flags=0, kB=KB):
        self.lib = _lib.load()
        group, ngroups = integrator._resolve_groups(system.num_particles)
        self.group, self.num_groups = group, ngroups
        n = system.num_particles
        self.n = n
        self.h = create_handle(self.lib, system, integrator, group, ngroups, _MODE[mode], _PREC[precision], -1, flags, kB,
                               (n + 31) // 32 * 32)

    def close(self):
        if getattr(self, "h", None):
            self.lib.tgnh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DrudeStatistics:
    """What HipContext.drude_statistics returns (read-only): pairs, over (pairs beyond `threshold`), max_distance and rms_distance
    (nm), worst_particle (slot of the Drude particle of the longest pair, -1: no pair), induced_dipole (e nm, 3 values), hist
    (int64, 33 values: 32 bins of width hist_max / 32, then the pairs at or beyond hist_max; zeros when hist_max == 0) and
    hist_edges (the 33 edges of the 32 bins; None when hist_max == 0)."""
    __slots__ = ("pairs", "over", "max_distance", "rms_distance", "worst_particle", "induced_dipole", "hist", "hist_edges",
                 "sum_d2", "threshold", "hist_max", "raw")

    def __init__(self, st, threshold, hist_max):
        put = lambda k, v: object.__setattr__(self, k, v)    # noqa: E731
        put("raw", bytes(st))                                # the struct as the library filled it in
        put("pairs", int(st.pairs)); put("over", int(st.over)); put("worst_particle", int(st.worst_particle))
        put("max_distance", float(st.max_distance)); put("sum_d2", float(st.sum_d2))
        put("rms_distance", float(np.sqrt(st.sum_d2 / st.pairs)) if st.pairs else 0.0)
        put("threshold", threshold); put("hist_max", hist_max)
        arrays = {"induced_dipole": np.array(st.dipole[:], np.float64), "hist": np.array(st.hist[:], np.int64),
                  "hist_edges": np.linspace(0.0, hist_max, _lib.DRUDE_HIST_BINS + 1) if hist_max > 0 else None}
        for k, v in arrays.items():
            if v is not None:
                v.setflags(write=False)
            put(k, v)

    def __setattr__(self, name, value):
        raise AttributeError("DrudeStatistics is read-only")

    def __repr__(self):
        return (f"DrudeStatistics(pairs={self.pairs}, over={self.over}, max_distance={self.max_distance:.6g}, "
                f"rms_distance={self.rms_distance:.6g}, worst_particle={self.worst_particle}, induced_dipole={self.induced_dipole.tolist()})")


class Momentum:
    """What HipContext.momentum returns (read-only): mass (amu) and momentum (amu nm/ps, 3 values) of the context's massive slots,
    massive (their number) and velocity = momentum / mass, the centre-of-mass velocity (zeros when there is no mass)."""
    __slots__ = ("mass", "momentum", "massive", "velocity", "raw")

    def __init__(self, st):
        put = lambda k, v: object.__setattr__(self, k, v)    # noqa: E731
        put("raw", bytes(st))                                # the struct as the library filled it in
        put("mass", float(st.mass)); put("massive", int(st.massive))
        p = np.array(st.momentum[:], np.float64)
        v = p / st.mass if st.mass != 0 else np.zeros(3)
        for k, a in (("momentum", p), ("velocity", v)):
            a.setflags(write=False)
            put(k, a)

    def __setattr__(self, name, value):
        raise AttributeError("Momentum is read-only")

    def __repr__(self):
        return f"Momentum(mass={self.mass:.6g}, momentum={self.momentum.tolist()}, massive={self.massive}, velocity={self.velocity.tolist()})"


class MinimizeState:
    """What HipContext.minimizeEnergy and minimize_state return (read-only): tgnh_minimize_state as the last decision left it --
    iterations (updates made), uphill (resets), since_uphill, moving (this context's moving slots), converged (0 running, 1 the
    rms force is <= tolerance, -1 a sum was not finite), dt, alpha, power (f.v), ff, vv and rms_force (kJ/mol/nm)."""
    __slots__ = ("iterations", "uphill", "since_uphill", "moving", "converged", "dt", "alpha", "power", "ff", "vv", "rms_force", "raw")

    def __init__(self, st):
        put = lambda k, v: object.__setattr__(self, k, v)    # noqa: E731
        put("raw", bytes(st))                                # the struct as the library filled it in
        for k in ("iterations", "uphill", "since_uphill", "moving", "converged"):
            put(k, int(getattr(st, k)))
        for k in ("dt", "alpha", "power", "ff", "vv", "rms_force"):
            put(k, float(getattr(st, k)))

    def __setattr__(self, name, value):
        raise AttributeError("MinimizeState is read-only")

    def __repr__(self):
        return (f"MinimizeState(iterations={self.iterations}, converged={self.converged}, rms_force={self.rms_force:.6g}, "
                f"uphill={self.uphill}, dt={self.dt:.6g}, alpha={self.alpha:.6g}, moving={self.moving})")


FIRE_DEFAULTS = dict(dt_start=1e-4, dt_max=1e-3, max_step=0.01, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99, n_min=5)


def minimize_desc(n, tolerance=10.0, drude_only=False, moving=None, **fire):
    """-> (tgnh_minimize_desc, the mask array it points to or None: keep it alive for the call).  **fire: FIRE_DEFAULTS' names."""
    unknown = set(fire) - set(FIRE_DEFAULTS)
    if unknown:
        raise TgnhError(_lib.ERR_ARG, f"minimize: unknown FIRE parameter(s) {sorted(unknown)}")
    par = dict(FIRE_DEFAULTS, **fire)
    d = _lib.TgnhMinimizeDesc()
    d.tolerance = float(tolerance)
    for k, v in par.items():
        setattr(d, k, int(v) if k == "n_min" else float(v))
    d.flags = _lib.MIN_DRUDE_ONLY if drude_only else 0
    mask = None
    if moving is not None:
        mask = np.ascontiguousarray(np.asarray(moving) != 0, np.uint8)
        if mask.shape != (n,):
            raise TgnhError(_lib.ERR_ARG, "minimize: one mask entry per particle slot")
        d.moving = mask.ctypes.data
    return d, mask


class HipContext(_HandleQueries):
    """Device state + handle: what OpenMM's Context / HIP platform data are to the reference kernel.

    force_fn(ctx) is the force call-out (calcForcesAndEnergy); the default is the
    harness force (Drude spring + tether) computed by the library's own kernel.
    cm_motion_removal: None = no centre-of-mass removal inside the step loops, whatever system.has_cm_motion_remover says (that
    flag only takes three degrees of freedom off the thermostats); an integer = tgnh_set_cm_motion_removal(every).
    direct_constraints: True hands the system's clusters of at most three constraints to the library's direct solver
    (split_clusters, tgnh_set_constraint_clusters) and only the rest to the harness' SHAKE; False (the default): all to the harness.
    library_sites: True hands the system's three-particle-average sites to the library's own site table (tgnh_set_virtual_sites)
    instead of the harness'; False (the default): to the harness.  A system's set_site_table goes to the library's table either way.
    site_forces (an attribute, default False): True lets every compute_forces() end with one distribute_site_forces(), for a force_fn
    that leaves forces on sites; the harness' water force spreads its M site's force itself and wants it off.
    drude_force (an attribute, default False): True lets every compute_forces() add the library's own DrudeForce
    (compute_drude_force()) after force_fn and before the sites' forces are spread.  A system that carries a forces.DrudeForce
    (DrudeSystem.set_drude_force) hands it to the handle here; nothing is launched for it until the attribute is set or
    compute_drude_force() is called.
    """
    _only_library_sites = False            # (minimizeEnergy: a context that says nothing else about itself is refused as a constrained one)

    def __init__(self, system, integrator, mode="TGNH", precision="mixed", device=0, flags=0, kB=KB,
                 k_drude=None, k_tether=None, allreduce=None, global_dof_sum=None, lattice_sites=True, cm_motion_removal=None,
                 direct_constraints=False, library_sites=False):
        import torch
        self.torch = torch
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise RuntimeError("the DrudeTGNH HIP path needs a GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.system, self.integrator = system, integrator
        self.mode, self.precision = _MODE[mode], _PREC[precision]
        self.dev = torch.device("cuda", device)
        n = system.num_particles
        self.n = n
        self.padded = (n + 31) // 32 * 32                    # OpenMM PADDED_NUM_ATOMS (TileSize 32)
        group, ngroups = integrator._resolve_groups(n)
        self.group, self.num_groups = group, ngroups
        from .synth import K_DRUDE, K_TETHER
        self.k_drude = K_DRUDE if k_drude is None else k_drude
        self.k_tether = K_TETHER if k_tether is None else k_tether

        with torch.cuda.device(self.dev):
            h = create_handle(self.lib, system, integrator, group, ngroups, self.mode, self.precision, device, flags, kB,
                              self.padded)
        self.h = h
        self._pushed_baths = (integrator.getTemperature(), integrator.getDrudeTemperature())   # what the handle was created at
        self._bath_epoch = 0
        self.first_particle = 0                              # a shard: the index of its first slot in the whole system (setVelocitiesToTemperature)
        self._hook = None
        self.cm_motion_removal = 0
        self.velocity_rescaling = 0
        if cm_motion_removal is not None:
            with torch.cuda.device(self.dev):
                self.set_cm_motion_removal(cm_motion_removal)
        if global_dof_sum is not None:                      # particle sharding: dof terms are additive over ranks
            self.set_global_dof_terms(global_dof_sum(self.local_dof_terms()))
        if allreduce is not None:
            self.set_allreduce(allreduce)

        rdt = torch.float32 if self.precision != PREC_DOUBLE else torch.float64
        mdt = torch.float32 if self.precision == PREC_SINGLE else torch.float64
        self.rdt, self.mdt = rdt, mdt
        self.posq = torch.zeros((n, 4), dtype=rdt, device=self.dev)
        self.posq_corr = torch.zeros((n, 4), dtype=torch.float32, device=self.dev) if self.precision == PREC_MIXED else None
        self.velm = torch.zeros((n, 4), dtype=mdt, device=self.dev)
        self.force = torch.zeros(3 * self.padded, dtype=torch.int64, device=self.dev)
        self.pos_delta = torch.zeros((n, 4), dtype=mdt, device=self.dev)
        self.x0 = torch.zeros((n, 4), dtype=rdt, device=self.dev)        # harness tether sites, w = tether flag
        self.sites_packed = False
        self.unpacked_sites = False                                      # (tests: the harness force from x0 itself, the round-1 kernel)
        self.use_lattice_sites = bool(lattice_sites)                     # (tests: False keeps the packed sites where the lattice form would hold)
        inv = np.where(system.mass == 0.0, 0.0, 1.0 / np.where(system.mass == 0.0, 1.0, system.mass))
        self.velm[:, 3] = torch.from_numpy(inv).to(self.dev, mdt)
        _check(self.lib.tgnh_bind_buffers(self.h, self.posq.data_ptr(),
                                          self.posq_corr.data_ptr() if self.posq_corr is not None else None,
                                          self.velm.data_ptr(), self.force.data_ptr(), self.pos_delta.data_ptr()))
        integrator._context = self
        self.force_fn = None
        self.state_hook = None
        self.ke_sum_valid = False
        self.constrained = False
        self._has_clusters = system.cluster_atoms is not None and len(system.cluster_atoms) > 0
        self._harness_clusters = 0
        if self._has_clusters:
            harness = (system.cluster_atoms, system.cluster_dist)
            if direct_constraints:
                direct, harness = split_clusters(*harness)
                self.set_constraint_clusters(*direct)
            self._harness_clusters = len(harness[0])
            if self._harness_clusters:
                _check(self.lib.tgnh_harness_set_clusters(self.h, len(harness[0]), harness[0].ctypes.data_as(_lib.c_i32p),
                                                          harness[1].ctypes.data_as(_lib.c_f64p)))
            self.constrained = True
        self.site_forces = False           # True: every compute_forces() is followed by one distribute_site_forces()
        self.drude_force = False           # True: every compute_forces() adds the library's DrudeForce after force_fn (compute_drude_force)
        self._harness_sites = False        # the harness' site table holds sites (the system's three-particle averages, unless library_sites)
        table = [np.zeros(0, np.int32), np.zeros((0, 4), np.int32), np.zeros((0, _lib.SITE_PARAMS))]     # what goes to the library's table
        if system.site_table_kinds is not None and len(system.site_table_kinds):
            table = [system.site_table_kinds, system.site_table_atoms, system.site_table_params]
        if system.site_atoms is not None and len(system.site_atoms):
            if library_sites:
                params = np.zeros((len(system.site_atoms), _lib.SITE_PARAMS))
                params[:, :3] = system.site_weights
                table = [np.concatenate([table[0], np.full(len(system.site_atoms), _lib.SITE_THREE_AVERAGE, np.int32)]),
                         np.concatenate([table[1], system.site_atoms]), np.concatenate([table[2], params])]
            else:
                _check(self.lib.tgnh_harness_set_virtual_sites(self.h, len(system.site_atoms),
                                                               system.site_atoms.ctypes.data_as(_lib.c_i32p),
                                                               system.site_weights.ctypes.data_as(_lib.c_f64p)))
                self._harness_sites = True
            self.constrained = True        # the split path is the one with the virtual-site call-out
        self._only_library_sites = not self._has_clusters and not self._harness_sites     # what makes the context `constrained` is at most sites of the library's table
        if len(table[0]):
            self.set_virtual_sites(*table)
        if system.drude_force is not None:
            self.set_drude_force(system.drude_force)
        if system.positions is not None:
            self.setPositions(system.positions)
            self.set_sites(system.positions)
        if system.velocities is not None:
            self.setVelocities(system.velocities)
        if system.positions is not None:
            self.compute_forces()

    # ---- plumbing ----
    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _push_scalars(self):
        i = self.integrator
        _check(self.lib.tgnh_set_step_size(self.h, i.getStepSize()))
        _check(self.lib.tgnh_set_drude_steps_per_real_step(self.h, i.getDrudeStepsPerRealStep()))
        _check(self.lib.tgnh_set_max_drude_distance(self.h, i.getMaxDrudeDistance()))
        baths = (i.getTemperature(), i.getDrudeTemperature())
        if baths != self._pushed_baths:                      # (only then: a run that never retargets makes no such call)
            _check(self.lib.tgnh_set_temperatures(self.h, baths[0], baths[1], self._stream()))
            self._pushed_baths = baths
            self._bath_epoch += 1                            # (capture_steps: a recorded step holds the old kT)

    def close(self):
        if getattr(self, "h", None):
            self.torch.cuda.synchronize(self.dev)
            self.lib.tgnh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_allreduce(self, fn):
        """fn(tensor_view) must sum the float64 device tensor in place over all ranks (stream-ordered)."""
        torch = self.torch

        def _hook(buf, count, stream, user):
            try:
                t = self._ke_view(buf, count)
                fn(t)
                return 0
            except Exception as e:     # never unwind through C
                print("all-reduce hook failed:", e)
                return 1
        self._hook = _lib.ALLREDUCE_FN(_hook)
        self._views = {}
        _check(self.lib.tgnh_set_allreduce(self.h, self._hook, None))

    # ---- the library's own RCCL all-reduce (include/drude_tgnh.h: tgnh_rccl_*) ----
    RCCL_ID_BYTES = 128

    def rccl_init(self, world, rank, unique_id):
        """Collective: every rank of `world` calls this with rank 0's id (rccl_unique_id())."""
        _check(self.lib.tgnh_rccl_init(self.h, int(world), int(rank), C.c_char_p(unique_id)))
        self._hook = None

    def rccl_unique_id(self):
        buf = C.create_string_buffer(self.RCCL_ID_BYTES)
        _check(self.lib.tgnh_rccl_unique_id(buf))
        return buf.raw

    def rccl_shutdown(self):
        _check(self.lib.tgnh_rccl_shutdown(self.h))

    def rccl_init_over(self, dist, rank, world):
        """The library's communicator set up through a torch.distributed process group (which only carries the 128-byte id):
        all ranks return True (the library enqueues ncclAllReduce itself from now on) or all return False (nothing changed)."""
        ok, err = 1, None
        ids = [None]
        # ncclCommInitRank is collective: a rank that cannot even bind RCCL must say so BEFORE anybody enters it, or its peers
        # wait inside it for good.  Every rank therefore makes an id of its own first (binds the library, not collective) and
        # the ranks vote; only rank 0's id is used.
        try:
            mine = self.rccl_unique_id()
            if rank == 0:
                ids[0] = mine
        except Exception as e:                      # noqa: BLE001
            ok, err = 0, e
        votes = [None] * world
        dist.all_gather_object(votes, ok)
        if not all(votes):
            self.rccl_error = err or RuntimeError("RCCL could not be bound on rank(s) " + str([r for r, v in enumerate(votes) if not v]))
            return False
        dist.broadcast_object_list(ids, src=0)
        try:
            self.rccl_init(world, rank, ids[0])
        except Exception as e:                      # noqa: BLE001
            ok, err = 0, e
        flags = [None] * world
        dist.all_gather_object(flags, ok)
        if not all(flags):
            if ok:
                self.rccl_shutdown()
            self.rccl_error = err
            return False
        return True

    # ---- mailbox exchange over xGMI (include/drude_tgnh.h: tgnh_exchange_*) ----
    XCHG_HANDLE_BYTES = 64

    def exchange_wait_stats(self):
        """(mean us, max us, exchanges) of this rank's waits for its peers' sums since the last call; resets."""
        mean, mx, n = C.c_double(), C.c_double(), C.c_int64()
        _check(self.lib.tgnh_exchange_wait_stats(self.h, self._stream(), C.byref(mean), C.byref(mx), C.byref(n)))
        return mean.value, mx.value, n.value

    def exchange_create(self, world, rank):
        """-> (IPC handle bytes for peers in other processes, device pointer for peers in this process)"""
        buf = C.create_string_buffer(self.XCHG_HANDLE_BYTES)
        ptr = C.c_void_p()
        _check(self.lib.tgnh_exchange_create(self.h, int(world), int(rank), buf, C.byref(ptr)))
        return buf.raw, ptr.value

    def exchange_attach(self, handles):
        """handles: every rank's IPC handle bytes, in rank order (own entry ignored)."""
        blob = b"".join(handles)
        _check(self.lib.tgnh_exchange_attach(self.h, blob))

    def exchange_attach_pointers(self, pointers):
        arr = (C.c_void_p * len(pointers))(*[C.c_void_p(p) for p in pointers])
        _check(self.lib.tgnh_exchange_attach_pointers(self.h, arr))

    def set_resident_share(self, share):
        """FLAG_RESIDENT_STEP: this context may fill 1/share of the device (several contexts stepping concurrently)."""
        _check(self.lib.tgnh_set_resident_share(self.h, int(share)))

    def resident_work_groups(self):
        """Work-groups per compute unit found resident together at create, of the kernel resident_kernel() names (0: the deferred
        launches run)."""
        n = C.c_int()
        _check(self.lib.tgnh_get_resident_work_groups(self.h, C.byref(n)))
        return n.value

    def resident_kernel(self):
        """The kernel the next step_begin runs as its one launch: None, 'step_kernel' or 'wstep_kernel'."""
        n = C.c_int()
        _check(self.lib.tgnh_get_resident_kernel(self.h, C.byref(n)))
        return (None, "step_kernel", "wstep_kernel")[n.value]

    def exchange_detach(self):
        _check(self.lib.tgnh_exchange_detach(self.h))

    def attach_exchange_over(self, dist, rank, world, tensor_device="cuda"):
        """Collective over a torch.distributed process group: every rank creates its mailbox, the hipIpc handles go
        round with all_gather_object, every rank maps its peers.  All ranks return the same answer: True = the
        mailbox exchange is attached everywhere; False = nowhere (a rank could not create / map: the all-reduce hook,
        if set, keeps doing the exchange)."""
        torch = self.torch
        ok, err = 1, None
        try:
            handle, _ = self.exchange_create(world, rank)
            handles = [None] * world
            dist.all_gather_object(handles, handle)
            self.exchange_attach(handles)
        except Exception as e:                      # noqa: BLE001 -- any failure means "not here", decided collectively below
            ok, err = 0, e
        t = torch.tensor([ok], dtype=torch.int32, device=tensor_device)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        if int(t.item()) == 0:
            if ok:
                self.exchange_detach()
            self.exchange_error = err
            return False
        return True

    def _ke_view(self, ptr, count):
        key = (ptr, count)
        v = self._views.get(key)
        if v is None:
            torch = self.torch

            class _Holder:
                pass
            hold = _Holder()
            hold.__cuda_array_interface__ = {"shape": (count,), "typestr": "<f8", "data": (ptr, False), "version": 2}
            v = torch.as_tensor(hold, device=self.dev)
            self._views[key] = v
        return v

    # ---- state (Context::setPositions / setVelocities / getState) ----
    def setPositions(self, pos):
        torch = self.torch
        self._state_changed()
        p = torch.from_numpy(np.ascontiguousarray(pos, np.float64)).to(self.dev)
        if self.precision == PREC_DOUBLE:
            self.posq[:, :3] = p
        else:
            hi = p.to(torch.float32)
            self.posq[:, :3] = hi
            if self.posq_corr is not None:
                self.posq_corr[:, :3] = (p - hi.to(torch.float64)).to(torch.float32)

    def set_sites(self, x0):
        """Harness tether sites (stored in the position type, so float-rounded unless precision is double);
        every massive particle that is not a Drude particle is tethered."""
        self.x0[:, :3] = self.torch.from_numpy(np.ascontiguousarray(x0, np.float64)).to(self.dev, self.rdt)
        flag = (self.system.mass > 0)
        flag[self.system.pair_drude] = False
        self.x0[:, 3] = self.torch.from_numpy(flag.astype(np.float64)).to(self.dev, self.rdt)
        self.torch.cuda.synchronize(self.dev)
        lat = getattr(self.system, "lattice", None)
        if lat is not None and self.use_lattice_sites:
            # (a hint only: the library checks every slot against it and packs the sites as before where it does not hold)
            k, side, spacing, geom, first = lat
            geom = np.ascontiguousarray(geom, np.float64)
            _check(self.lib.tgnh_harness_lattice_hint(self.h, int(k), int(side), float(spacing), geom.ctypes.data_as(_lib.c_f64p), int(first)))
        else:
            _check(self.lib.tgnh_harness_lattice_hint(self.h, 0, 0, 0.0, None, 0))
        _check(self.lib.tgnh_harness_pack_sites(self.h, self.x0.data_ptr()))
        self.sites_packed = True

    def sites_kind(self):
        """how the harness force finds its tether sites: 'x0' (explicit array), 'packed', 'lattice'"""
        n = C.c_int()
        _check(self.lib.tgnh_harness_sites_kind(self.h, C.byref(n)))
        return ("x0", "packed", "lattice")[n.value]

    def _x0_arg(self):
        """None (NULL: the library reads its packed copy) once set_sites has packed them, else the float4 / double4 array"""
        return None if self.sites_packed and not self.unpacked_sites else self.x0.data_ptr()

    def sites(self):
        """The tether sites exactly as the harness kernel sees them (for the oracle)."""
        return self.x0[:, :3].to(self.torch.float64).cpu().numpy()

    def setVelocities(self, vel):
        self._state_changed()                                # (first: refused between the steps of a deferred sequence, and then nothing is written)
        self.velm[:, :3] = self.torch.from_numpy(np.ascontiguousarray(vel, np.float64)).to(self.dev, self.mdt)

    def rebind_velocities(self, velm):
        """tgnh_bind_buffers with another velm array (same shape, type and device) and every other array as bound; the context
        steps on it from here on.  Refused (TGNH_ERR_STATE) while a deferred half kick is pending: flush first, or call it between
        step_begin and step_end.  The array that goes holds the current velocities when the call returns; what the new one holds
        is the caller's business (its w must be 1/m)."""
        if velm.shape != self.velm.shape or velm.dtype != self.velm.dtype or velm.device != self.velm.device or not velm.is_contiguous():
            raise TgnhError(_lib.ERR_ARG, "rebind_velocities: a contiguous array of velm's shape, type and device")
        _check(self.lib.tgnh_bind_buffers(self.h, self.posq.data_ptr(),
                                          self.posq_corr.data_ptr() if self.posq_corr is not None else None,
                                          velm.data_ptr(), self.force.data_ptr(), self.pos_delta.data_ptr()))
        old, self.velm = self.velm, velm
        return old

    # ---- centre-of-mass motion (include/drude_tgnh.h: tgnh_get_momentum, tgnh_remove_cm_motion, ...) ----
    def momentum(self):
        """tgnh_get_momentum: total mass and momentum of this context's slots, summed on the device (what a step left owed to the
        velocities is applied first).  Synchronises the stream.  In a sharded run every context answers for its own slots; the
        fields add up over ranks."""
        st = _lib.TgnhMomentum()
        st.struct_size = C.sizeof(st)
        _check(self.lib.tgnh_get_momentum(self.h, self._stream(), C.byref(st)))
        return Momentum(st)

    def removeCMMotion(self):
        """tgnh_remove_cm_motion: v -= P / M on every massive slot, on the device and without a host synchronisation; with an
        all-reduce set (set_allreduce, rccl_init) P and M are the whole system's, and the call is collective."""
        _check(self.lib.tgnh_remove_cm_motion(self.h, self._stream()))
        self.ke_sum_valid = False

    def shift_velocities(self, dv):
        """tgnh_shift_velocities: v -= dv on every massive slot."""
        dv = np.ascontiguousarray(dv, np.float64)
        if dv.shape != (3,):
            raise TgnhError(_lib.ERR_ARG, "shift_velocities: dv must have three components")
        _check(self.lib.tgnh_shift_velocities(self.h, dv.ctypes.data_as(_lib.c_f64p), self._stream()))
        self.ke_sum_valid = False

    def set_cm_motion_removal(self, every):
        """tgnh_set_cm_motion_removal: remove the centre-of-mass motion before every step whose number is a multiple of `every`
        (0: off), inside step() and whatever else runs the step entry points."""
        _check(self.lib.tgnh_set_cm_motion_removal(self.h, int(every)))
        self.cm_motion_removal = int(every)

    # ---- velocity rescaling (include/drude_tgnh.h: tgnh_scale_velocities, tgnh_rescale_to_temperature, ...) ----
    def _bath_pair(self, temperature, drudeTemperature):
        return (float(self.integrator.getTemperature() if temperature is None else temperature),
                float(self.integrator.getDrudeTemperature() if drudeTemperature is None else drudeTemperature))

    def scale_velocities(self, factors):
        """tgnh_scale_velocities: the integrator's own rescale with one factor per thermostat, in last_scale_factors()' layout
        (TGNH [groups.., COM, Drude], dualNH [real, unused, Drude]): velocities relative to their molecule's centre of mass by
        their group's factor, the centres of mass by theirs, the relative Drude motion by the Drude factor.  No host
        synchronisation; `factors` is read before the call returns."""
        f = np.ascontiguousarray(factors, np.float64)
        if f.ndim != 1:
            raise TgnhError(_lib.ERR_ARG, "scale_velocities: factors must be a vector, one per thermostat")
        _check(self.lib.tgnh_scale_velocities(self.h, f.ctypes.data_as(_lib.c_f64p), len(f), self._stream()))
        self.ke_sum_valid = False

    def rescale_to_temperature(self, temperature=None, drudeTemperature=None):
        """tgnh_rescale_to_temperature: every thermostat's kinetic energy onto N kT at these temperatures (default: the
        integrator's) -- kinetic-energy pass, all-reduce where one is set (the call is then collective), factors, rescale, all on
        the device.  The baths stay as they are.  last_kinetic_energies() has the sums before scaling, rescale_factors() the
        factors."""
        _check(self.lib.tgnh_rescale_to_temperature(self.h, *self._bath_pair(temperature, drudeTemperature), self._stream()))
        self.ke_sum_valid = False

    def rescale_factors(self):
        """tgnh_get_rescale_factors: what the last scale_velocities / rescale_to_temperature applied.  Synchronises the stream."""
        return self._vec(self.lib.tgnh_get_rescale_factors, self.num_thermostats())

    def set_velocity_rescaling(self, every, temperature=None, drudeTemperature=None):
        """tgnh_set_velocity_rescaling: rescale_to_temperature before every step whose number is a multiple of `every` (0: off),
        after a centre-of-mass removal due at the same step, inside step() and whatever else runs the step entry points."""
        _check(self.lib.tgnh_set_velocity_rescaling(self.h, int(every), *self._bath_pair(temperature, drudeTemperature)))
        self.velocity_rescaling = int(every)
        self.ke_sum_valid = False

    # ---- the barostat's trial move (include/drude_tgnh.h: tgnh_scale_positions, tgnh_restore_positions) ----
    def scale_positions(self, scale, save=False):
        """tgnh_scale_positions: every molecule of the table in force (set_molecules) moved rigidly by (scale - 1) x its centroid,
        about the origin; a scalar means isotropic.  save=True keeps what was read in a snapshot of the handle's
        (restore_positions), in the same launch.  No host synchronisation; velocities, thermostat and everything a step left
        pending stay as they are.  Refused while a half kick is owed to the velocities (flush() first).  The caller scales its own
        box and recomputes the forces before the next step."""
        sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, np.float64), (3,)) if np.ndim(scale) == 0 else scale, np.float64)
        if sc.shape != (3,):
            raise TgnhError(_lib.ERR_ARG, "scale_positions: scale is a scalar or has three components")
        _check(self.lib.tgnh_scale_positions(self.h, sc.ctypes.data_as(_lib.c_f64p), int(bool(save)), self._stream()))

    def restore_positions(self):
        """tgnh_restore_positions: the positions (and charges) as the last scale_positions(save=True) read them, bit for bit."""
        _check(self.lib.tgnh_restore_positions(self.h, self._stream()))

    # ---- energy minimisation (include/drude_tgnh.h: tgnh_minimize_begin, tgnh_minimize_iterate, ...) ----
    def minimize_begin(self, tolerance=10.0, drude_only=False, moving=None, **fire):
        """tgnh_minimize_begin: which slots move, the FIRE parameters (FIRE_DEFAULTS), and the minimiser's velocity -- a float64
        tensor [3, N] of this context's (self.minimize_work), zeroed by the call."""
        d, mask = minimize_desc(self.n, tolerance, drude_only, moving, **fire)
        self.minimize_work = self.torch.empty((3, self.n), dtype=self.torch.float64, device=self.dev)
        _check(self.lib.tgnh_minimize_begin(self.h, C.byref(d), self.minimize_work.data_ptr(), self._stream()))

    def minimize_iterate(self):
        """tgnh_minimize_iterate: one FIRE iteration on whatever the force buffer holds; no host synchronisation."""
        _check(self.lib.tgnh_minimize_iterate(self.h, self._stream()))

    def minimize_state(self):
        """tgnh_get_minimize_state.  Synchronises the stream."""
        st = _lib.TgnhMinimizeState()
        _check(self.lib.tgnh_get_minimize_state(self.h, self._stream(), C.byref(st)))
        return MinimizeState(st)

    def minimize_end(self):
        _check(self.lib.tgnh_minimize_end(self.h))
        self.minimize_work = None

    def _minimize_batch(self, iterations):
        """`iterations` x {virtual sites where the context has them, the force call-out, one iteration}, enqueued back to back"""
        sites = self._harness_sites or self.num_virtual_sites > 0
        if self.force_fn is None and not self.drude_force and not sites:      # (the C loop knows the harness force alone, as step()'s do)
            _check(self.lib.tgnh_run_harness_minimize(self.h, self._x0_arg(), self.k_drude, self.k_tether, int(iterations), self._stream()))
            return
        for _ in range(iterations):
            if sites:
                self._place_sites()
            self.compute_forces()
            self.minimize_iterate()

    def minimizeEnergy(self, tolerance=10.0, maxIterations=0, drude_only=False, moving=None, check_every=50, **fire):
        """OpenMM's Context.minimizeEnergy plus the Drude option, by FIRE on the device between force call-outs: until the root
        mean square of the moving slots' force components is <= tolerance (kJ/mol/nm), or for maxIterations iterations (0: until
        converged).  drude_only=True moves only the Drude particles (the relaxation a Drude system needs before its first step);
        moving: a mask, one entry per slot.  Massless slots never move.  The state is read back every check_every iterations;
        nothing else waits for the device.  **fire: FIRE_DEFAULTS' names.  Constraints are not projected: a constrained context
        is refused unless drude_only or a mask says which slots are free to move, and so is one whose virtual sites live in the
        harness' table; sites in the library's table (library_sites=True, set_virtual_sites) are placed before every force
        call-out and, with site_forces set, their forces spread after it, so every massive slot may move.  Velocities, thermostat and step count stay as
        they are.  Returns a MinimizeState; unless it says converged == 1 the forces are recomputed at the final positions."""
        # (sites in the library's table are placed before every force call-out and, with site_forces, their forces spread after it:
        # such a context may move every massive slot; constraints, and sites in the harness' table, are refused as before)
        if self.constrained and not self._only_library_sites and not drude_only and moving is None:
            raise TgnhError(_lib.ERR_STATE, "minimizeEnergy: the context has constraints or virtual sites and the minimiser projects no "
                                            "constraints: pass drude_only=True or a `moving` mask of slots that no constraint touches")
        if check_every < 1 or maxIterations < 0:
            raise TgnhError(_lib.ERR_ARG, "minimizeEnergy: check_every must be positive and maxIterations not negative")
        self.flush()
        self.minimize_begin(tolerance, drude_only, moving, **fire)
        try:
            done = 0
            while True:
                batch = int(check_every) if maxIterations == 0 else min(int(check_every), int(maxIterations) - done)
                if batch > 0:
                    self._minimize_batch(batch)
                    done += batch
                st = self.minimize_state()
                if st.converged != 0 or batch <= 0 or (maxIterations and done >= maxIterations):
                    break
        finally:
            self.minimize_end()
        if st.converged != 1:                                # (the buffer holds the forces of the positions before the last update)
            self._place_sites()
            self.compute_forces()
        return st

    # ---- whole molecules back into the cell, and frames for a trajectory file (tgnh_wrap_molecules, tgnh_write_frame) ----
    def wrap_molecules(self):
        """tgnh_wrap_molecules: every molecule of the table in force whose centroid lies outside the cell [0, L) of the box
        (setPeriodicBoxVectors) moved by whole box vectors, on the device; a molecule inside is not written at all.  No host
        synchronisation, no flush needed; velocities, thermostat and everything a step left pending stay as they are.  Not for a
        run on the harness force: its tether is not periodic."""
        _check(self.lib.tgnh_wrap_molecules(self.h, self._stream()))

    def frame(self, wrap=False, skip_drude=False, unit=1.0, planes=False, out=None):
        """tgnh_write_frame: the positions as a float32 tensor on the device, [count, 3] -- or [3, count] with planes=True, what a
        DCD record is --, every coordinate times `unit` (10.0: Angstrom), formed in fp64 and rounded once.  wrap=True: as
        wrap_molecules() would leave them, without touching the positions.  skip_drude=True leaves the Drude particles out
        (count = frame_count(True)).  One read-only launch on the current stream; nothing is copied to the host.  out: a
        contiguous float32 tensor of that shape on the context's device to write into."""
        torch = self.torch
        count = self.frame_count(skip_drude)
        shape = (3, count) if planes else (count, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.dev)
        elif out.dtype != torch.float32 or out.device != self.dev or tuple(out.shape) != shape or not out.is_contiguous():
            raise TgnhError(_lib.ERR_ARG, f"frame: out must be a contiguous float32 tensor of shape {shape} on {self.dev}")
        d = _lib.TgnhFrameDesc()
        d.struct_size = C.sizeof(d)
        d.flags = (_lib.FRAME_WRAP if wrap else 0) | (_lib.FRAME_SKIP_DRUDE if skip_drude else 0) | (0 if planes else _lib.FRAME_INTERLEAVED)
        d.unit, d.stride, d.capacity = float(unit), count if planes else 0, 3 * count
        _check(self.lib.tgnh_write_frame(self.h, C.byref(d), out.data_ptr(), self._stream()))
        return out

    def setVelocitiesToTemperature(self, temperature, randomSeed=None, drudeTemperature=None, removeCMMotion=False, exact=False):
        """OpenMM's Context.setVelocitiesToTemperature, Drude-aware and drawn on the device (tgnh_set_velocities_to_temperature):
        pair centres of mass and ordinary particles at `temperature`, the relative Drude motion at `drudeTemperature` (default:
        the integrator's).  randomSeed=None takes one from os.urandom; the same seed gives the same velocities on any handle,
        path or sharding (self.first_particle places a shard in the whole system).  With constraint clusters set, the harness'
        velocity-constraint stage and the direct solver's run afterwards, as OpenMM projects after its draw.  removeCMMotion=True takes the net momentum
        the draw leaves (of order sqrt(N) thermal momenta) off again, after that stage (removeCMMotion()).  exact=True then puts
        every thermostat's kinetic energy onto its N kT at these temperatures, last of all (rescale_to_temperature())."""
        if drudeTemperature is None:
            drudeTemperature = self.integrator.getDrudeTemperature()
        if randomSeed is None:
            import os
            randomSeed = int.from_bytes(os.urandom(8), "little")
        seed = int(randomSeed) & 0xFFFFFFFFFFFFFFFF
        seed = seed - (1 << 64) if seed >> 63 else seed      # (the same 64 bits as a c_int64)
        _check(self.lib.tgnh_set_velocities_to_temperature(self.h, float(temperature), float(drudeTemperature), seed,
                                                           int(self.first_particle), self._stream()))
        self.ke_sum_valid = False
        if self._has_clusters:
            _check(self.lib.tgnh_harness_shake_velocities(self.h, self.integrator.getConstraintTolerance(), self._stream()))
            _check(self.lib.tgnh_apply_velocity_constraints(self.h, self.integrator.getConstraintTolerance(), self._stream()))
        if removeCMMotion:
            self.removeCMMotion()
        if exact:
            self.rescale_to_temperature(temperature, drudeTemperature)

    @property
    def constraint_clusters(self):
        """(direct, harness): the clusters in the direct solver's table and in the harness' SHAKE table"""
        return self.num_constraint_clusters(), self._harness_clusters

    def apply_constraints(self, tol=None):
        """tgnh_apply_constraints: the direct solver on posDelta, for the clusters of its table (tol=None: the integrator's
        constraint tolerance; it gates the result, status bit 1, and does not steer the solve).  No synchronisation."""
        tol = self.integrator.getConstraintTolerance() if tol is None else float(tol)
        _check(self.lib.tgnh_apply_constraints(self.h, tol, self._stream()))

    def apply_velocity_constraints(self, tol=None):
        """tgnh_apply_velocity_constraints: the direct solver's velocity stage on velm (one linear solve per cluster)."""
        tol = self.integrator.getConstraintTolerance() if tol is None else float(tol)
        _check(self.lib.tgnh_apply_velocity_constraints(self.h, tol, self._stream()))
        self.ke_sum_valid = False

    # ---- the library's own virtual-site stage (include/drude_tgnh.h: tgnh_set_virtual_sites, ...) ----
    def set_virtual_sites(self, kinds, atoms, params):
        """tgnh_set_virtual_sites (see _HandleQueries.set_virtual_sites); a context with sites steps along the split path, the one
        with the virtual-site call-out."""
        super().set_virtual_sites(kinds, atoms, params)
        if self.num_virtual_sites:
            self.constrained = True

    def compute_virtual_sites(self):
        """tgnh_compute_virtual_sites: every site of the library's table placed from its parents.  No synchronisation."""
        _check(self.lib.tgnh_compute_virtual_sites(self.h, self._stream()))

    def distribute_site_forces(self):
        """tgnh_distribute_virtual_site_forces on the context's force buffer: what the buffer holds on sites is spread over their
        parents (and left on the sites, which have no mass: a second call adds a second time).  No synchronisation."""
        _check(self.lib.tgnh_distribute_virtual_site_forces(self.h, self.force.data_ptr(), self._stream()))

    # ---- the library's own DrudeForce (include/drude_tgnh.h: tgnh_set_drude_force, ...) ----
    def compute_drude_force(self, energy=False):
        """tgnh_compute_drude_force on the context's force buffer: the springs, their anisotropy and the screened pairs of the table
        in force are ADDED to what the buffer holds (an empty table: no launch).  energy=True: the same launch leaves the partial
        sums drude_energy() adds.  No synchronisation."""
        _check(self.lib.tgnh_compute_drude_force(self.h, self.force.data_ptr(), 1 if energy else 0, self._stream()))

    def drude_energy(self):
        """tgnh_get_drude_energy: (springs, screened pairs) in kJ/mol, of the positions the last compute_drude_force(energy=True)
        read.  Synchronises."""
        out = np.zeros(2)
        _check(self.lib.tgnh_get_drude_energy(self.h, self._stream(), out.ctypes.data_as(_lib.c_f64p)))
        return float(out[0]), float(out[1])

    def _place_sites(self):
        """the virtual-site call-out (Cu :377): the harness' table where it holds sites, then the library's (none: no launch)"""
        if self._harness_sites:
            _check(self.lib.tgnh_harness_virtual_sites(self.h, self._stream()))
        _check(self.lib.tgnh_compute_virtual_sites(self.h, self._stream()))

    def setCharges(self, q):
        """posq.w of every slot (OpenMM keeps the charge there; setPositions leaves it alone).  No step kernel reads it."""
        self.posq[:, 3] = self.torch.from_numpy(np.ascontiguousarray(q, np.float64)).to(self.dev, self.rdt)

    def _state_changed(self):                                # DrudeTGNHIntegrator.cpp:166-170
        self.ke_sum_valid = False
        _check(self.lib.tgnh_state_changed(self.h))

    def getPositions(self):
        p = self.posq[:, :3].to(self.torch.float64)
        if self.posq_corr is not None:
            p = p + self.posq_corr[:, :3].to(self.torch.float64)
        return p.cpu().numpy()

    def flush(self):
        """velm <- the reference's end-of-step velocities (a deferred variant's pending half kick and factors applied)"""
        _check(self.lib.tgnh_flush(self.h, self._stream()))

    def getVelocities(self):
        _check(self.lib.tgnh_flush(self.h, self._stream()))
        return self.velm[:, :3].to(self.torch.float64).cpu().numpy()

    def getForces(self):
        f = self.force.view(3, self.padded)[:, :self.n].to(self.torch.float64) / 4294967296.0
        return f.t().contiguous().cpu().numpy()

    def setForces(self, f):
        """Forces in kJ/mol/nm -> OpenMM fixed point (long long)(f * 2^32)."""
        t = self.torch.from_numpy(np.ascontiguousarray(f, np.float64)).to(self.dev)
        self.force.view(3, self.padded)[:, :self.n] = (t * 4294967296.0).to(self.torch.int64).t()

    # ---- the step ----
    def compute_forces(self):
        if self.force_fn is not None:
            self.force_fn(self)
        else:
            _check(self.lib.tgnh_harness_force(self.h, self._x0_arg(), self.k_drude, self.k_tether,
                                               self.force.data_ptr(), self._stream()))
        if self.drude_force:
            self.compute_drude_force()
        if self.site_forces:
            self.distribute_site_forces()

    def step_begin(self):
        _check(self.lib.tgnh_step_begin(self.h, self._stream()))

    def step_end(self):
        _check(self.lib.tgnh_step_end(self.h, self._stream()))
        self.ke_sum_valid = True                             # DrudeTGNHIntegrator.cpp:192

    def step(self, steps):
        harness_loop = self.force_fn is None and not self.drude_force      # (the C loops know the harness force alone)
        if harness_loop and self.constrained:
            _check(self.lib.tgnh_run_harness_constrained(self.h, self._x0_arg(), self.k_drude, self.k_tether,
                                                         self.integrator.getConstraintTolerance(), int(steps), self._stream()))
            if steps > 0:
                self.ke_sum_valid = True
            return
        if harness_loop:
            _check(self.lib.tgnh_run_harness(self.h, self._x0_arg(), self.k_drude, self.k_tether, int(steps), self._stream()))
            if steps > 0:
                self.ke_sum_valid = True
            return
        # caller-supplied force call-out (and, optionally, a state hook: Context::updateContextState, e.g. CMMotionRemover)
        lib, h = self.lib, self.h
        for _ in range(steps):
            if self.state_hook is not None:
                self.state_hook(self)                                   # DrudeTGNHIntegrator.cpp:186
            if not self.constrained:
                self.step_begin()
                self.compute_forces()
                self.step_end()
                continue
            tol = self.integrator.getConstraintTolerance()
            _check(lib.tgnh_step_begin_kick(h, self._stream()))          # Cu :336-360
            _check(lib.tgnh_harness_shake_positions(h, tol, self._stream()))   # Cu :363
            _check(lib.tgnh_apply_constraints(h, tol, self._stream()))         # ... the direct solver's clusters
            _check(lib.tgnh_step_begin_move(h, self._stream()))          # Cu :366-376
            self._place_sites()                                          # Cu :377
            self.compute_forces()                                        # Cu :380
            _check(lib.tgnh_step_end_kick(h, self._stream()))            # Cu :384-388
            if self.mode == MODE_TGNH:
                _check(lib.tgnh_harness_shake_velocities(h, tol, self._stream()))   # Cu :391
                _check(lib.tgnh_apply_velocity_constraints(h, tol, self._stream()))
            _check(lib.tgnh_step_end_thermo(h, self._stream()))          # Cu :394-406
            self.ke_sum_valid = True

    def step_without_forces(self, steps):
        """`steps` x (step_begin, step_end) with NO force call-out, on whatever the force buffer holds: for timing the integrator's
        own launches (bench.py's integrator_only leg); not a trajectory of anything."""
        if self.constrained:
            raise TgnhError(_lib.ERR_STATE, "step_without_forces: unconstrained systems only")
        _check(self.lib.tgnh_run_steps(self.h, int(steps), self._stream()))
        if steps > 0:
            self.ke_sum_valid = True

    def capture_steps(self, steps, forces=True):
        """Captures `steps` time steps (harness force call-out included -- and the harness' constraint / virtual-site call-outs for a
        system with constraints --, and the KE all-reduce when sharded; forces=False: no call-out, see step_without_forces) into
        a hipGraph on a side stream and returns a callable that replays it.  The step sequence must not change afterwards
        (no setters).  A handle that is not in the steady state of its step sequence is brought there first, by up to
        three times `steps` real steps (see below): read the step count afterwards if it matters."""
        torch = self.torch
        if self.force_fn is not None or self.drude_force:
            raise TgnhError(_lib.ERR_STATE, "capture_steps supports the harness force call-out only")
        # A recording bakes in the centre-of-mass removals of the steps it recorded (set_cm_motion_removal): it replays the loop's
        # own launches only if every replay starts at a multiple of the interval, and so ends at one
        # (and the velocity rescalings, set_velocity_rescaling, alike)
        for what, every in (("centre-of-mass removal", self.cm_motion_removal), ("velocity rescaling", self.velocity_rescaling)):
            if every > 0 and (self.time()[1] % every or int(steps) % every):
                raise TgnhError(_lib.ERR_STATE, f"capture_steps: with {what} every {every} steps, the step count at the "
                                f"capture ({self.time()[1]}) and the steps captured ({int(steps)}) must both be multiples of it")
        # A graph replays launches, not the decisions that chose them: it may only be replayed from the state it was recorded
        # in.  The first steps of a handle differ from the later ones (nothing pending yet, a staged thermostat block to
        # commit), and so does a step after a query or a split step that settled part of what a step leaves owed.  So the
        # recording is checked: what the handle owes the trajectory (tgnh_get_pending_state) must be the same after the
        # recorded steps as before.  If it is not, the recording is a transition into the steady state: it is replayed once --
        # which takes exactly those steps, correctly, from the state they were recorded in -- and dropped, and the steps are
        # recorded again from where that leaves the handle.
        torch.cuda.synchronize(self.dev)
        # Consecutive streaming launches sweep the tiles in alternating directions, and a time step holds an odd number
        # of them: the launches of `steps` steps captured now and the launches of the `steps` steps after them differ in
        # that direction when `steps` is odd.  Two graphs are therefore captured back to back and replayed in turn, so a
        # replayed run issues exactly the launches the eager loop would (bitwise the same trajectory, for any `steps`).
        def record():
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                if self.constrained and not forces:
                    raise TgnhError(_lib.ERR_STATE, "capture_steps(forces=False): unconstrained systems only")
                if self.constrained:                         # the step loop step() runs for such a system: the split entry points around the harness' constraint call-outs
                    _check(self.lib.tgnh_run_harness_constrained(self.h, self._x0_arg(), self.k_drude, self.k_tether,
                                                                 self.integrator.getConstraintTolerance(), int(steps), self._stream()))
                elif not forces:
                    _check(self.lib.tgnh_run_steps(self.h, int(steps), self._stream()))
                else:
                    _check(self.lib.tgnh_run_harness(self.h, self._x0_arg(), self.k_drude, self.k_tether, int(steps), self._stream()))
            return g
        for _ in range(4):
            owed_before = self.pending_state() & 0x6ff
            first = record()
            if self.pending_state() & 0x6ff == owed_before:
                break
            first.replay()                                   # a transition: taken for real (the recording has advanced the clock)
            torch.cuda.synchronize(self.dev)
            self.ke_sum_valid = True
        else:
            raise TgnhError(_lib.ERR_STATE, "capture_steps: the handle does not reach a steady state of its step sequence")
        clock = self.time()
        graphs = [first, record()]
        if self.pending_state() & 0x6ff != owed_before:
            raise TgnhError(_lib.ERR_STATE, "capture_steps: the step sequence is not periodic")
        # a capture advances the host-side clock without running anything: the first one stands for the first replay,
        # the second one is taken back
        self.set_time(*clock)
        self._captured_not_run = int(steps)
        turn = [0]
        baths = self._bath_epoch

        planes = owed_before & 0x400

        def replay():
            # the launches of a recording read the velocities where they lived when it was made (bit 10: the one-launch step's own
            # planes, or velm): a query or a flush since has moved them, and a replay would step from stale ones
            if (self.pending_state() ^ planes) & 0x400:
                raise TgnhError(_lib.ERR_STATE, "capture_steps: the velocities no longer live where these steps were recorded "
                                "(a flush or a query moved them between the library's planes and velm): capture them again")
            if self._bath_epoch != baths:
                raise TgnhError(_lib.ERR_STATE, "capture_steps: the temperatures were changed after these steps were recorded "
                                "(their launches hold the old kT): capture them again")
            graphs[turn[0] & 1].replay()
            turn[0] += 1
            if self._captured_not_run:
                self._captured_not_run = 0          # first replay is the run the capture already counted
            else:
                _check(self.lib.tgnh_note_replayed_steps(self.h, int(steps)))
            self.ke_sum_valid = True
        replay.graph = graphs[0]
        replay.graphs = graphs
        return replay

    def pending_state(self):
        """tgnh_get_pending_state: what the handle still owes the trajectory (bit set, include/drude_tgnh.h)."""
        bits = C.c_uint32()
        _check(self.lib.tgnh_get_pending_state(self.h, C.byref(bits)))
        return bits.value

    def velocity_planes(self):
        """tgnh_get_velocity_planes: (live, usable, one-launch steps in a row since the last settle, the threshold) -- whether the
        one-launch step keeps the velocities in its own x | y | z planes right now, and whether this handle ever can."""
        out = (C.c_int32 * 4)()
        _check(self.lib.tgnh_get_velocity_planes(self.h, out))
        return bool(out[0]), bool(out[1]), int(out[2]), int(out[3])

    def status_flags(self):
        """The device's status word (bit 0 Drude beyond 2x the hard wall, bit 1 harness SHAKE not converged or the direct solver's result outside the tolerance, bit 2 mailbox
        exchange timed out), whether or not it spells a failure.  Synchronises the stream."""
        flags = C.c_uint32()
        self.lib.tgnh_get_status_flags(self.h, self._stream(), C.byref(flags))
        return flags.value

    def check(self):
        """The status word; raises TgnhError for the failures among its bits: a Drude beyond 2x the hard wall in dualNH
        mode (Ref :311-312), a mailbox exchange that timed out.  Once seen, a failure is sticky in the library: every
        later step or query raises too."""
        flags = C.c_uint32()
        _check(self.lib.tgnh_get_status_flags(self.h, self._stream(), C.byref(flags)))
        return flags.value

    # ---- queries ----
    def _vec(self, fn, n):
        out = np.zeros(n)
        _check(fn(self.h, self._stream(), out.ctypes.data_as(_lib.c_f64p)))
        return out

    def last_kinetic_energies(self):
        return self._vec(self.lib.tgnh_get_last_kinetic_energies, self.num_thermostats())

    def last_scale_factors(self):
        return self._vec(self.lib.tgnh_get_last_scale_factors, self.num_thermostats())

    def compute_kinetic_energies(self):
        _check(self.lib.tgnh_compute_kinetic_energies(self.h, self._stream()))
        return self.last_kinetic_energies()

    def half_kick(self):
        _check(self.lib.tgnh_half_kick(self.h, self._stream()))

    def kinetic_energy(self):
        out = C.c_double()
        _check(self.lib.tgnh_get_kinetic_energy(self.h, int(self.ke_sum_valid), self._stream(), C.byref(out)))
        return out.value

    def drude_statistics(self, threshold=None, hist_max=0.0):
        """tgnh_get_drude_statistics: the Drude-parent distances and the induced dipole of the positions as they are, summed on
        the device (no copy of the positions, no flush).  threshold=None: the integrator's getMaxDrudeDistance().  Synchronises
        the stream.  In a sharded run every context answers for its own slots (see include/drude_tgnh.h for what adds up)."""
        if threshold is None:
            threshold = self.integrator.getMaxDrudeDistance()
        st = _lib.TgnhDrudeStats()
        st.struct_size = C.sizeof(st)
        _check(self.lib.tgnh_get_drude_statistics(self.h, float(threshold), float(hist_max), self._stream(), C.byref(st)))
        return DrudeStatistics(st, float(threshold), float(hist_max))

    def time(self):
        t, k = C.c_double(), C.c_int64()
        _check(self.lib.tgnh_get_time(self.h, C.byref(t), C.byref(k)))
        return t.value, k.value

    def set_time(self, time, step_count):
        """Context::setTime / setStepCount of a restored checkpoint."""
        _check(self.lib.tgnh_set_time(self.h, float(time), int(step_count)))

    def timing(self, on):
        _check(self.lib.tgnh_timing_enable(self.h, int(on)))

    def timing_read(self, kid):
        ms, n = C.c_double(), C.c_int64()
        _check(self.lib.tgnh_timing_read(self.h, kid, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def algorithmic_bytes(self, kid):
        b = C.c_double()
        _check(self.lib.tgnh_algorithmic_bytes(self.h, kid, C.byref(b)))
        return b.value
