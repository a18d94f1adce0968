"""Forces the library computes itself, for a host that has no OpenMM behind it.

`DrudeForce` keeps the method names and argument order of OpenMM's DrudeForce (addParticle / addScreenedPair and their getters and
setters); it holds the table only.  `tables()` gives it in the form tgnh_set_drude_force takes (include/drude_tgnh.h has the
contract and the terms); `DrudeSystem.set_drude_force` attaches it to a system, and a `HipContext` over such a system hands it to
its handle.  Units are OpenMM's: charge e, polarizability nm^3.

`HarmonicBondForce`, `HarmonicAngleForce` and `PeriodicTorsionForce` are tables of the same kind with OpenMM's method names (nm, rad,
kJ/mol); `BondedForces` hands up to three of them to a handle (tgnh_set_bonded_forces) and is itself a force call-out:
`ctx.force_fn = BondedForces(ctx, bonds, angles, torsions)` with `ctx.drude_force = True` runs a flexible Drude molecule on the
library's forces alone.

`NonbondedForce` is OpenMM's table of charges, Lennard-Jones parameters and exceptions with its method names; `NonbondedForces` hands
it to a handle (tgnh_set_nonbonded_force: CutoffPeriodic with a reaction field, over cell lists) and is a force call-out too:
`BondedForces(ctx, ...).then(lambda c: nb.compute())`.  A table whose method is `Ewald` is handed over as CutoffPeriodic followed by
tgnh_set_nonbonded_ewald: an explicit reciprocal sum, O(n M), for boxes of up to a few ten thousand slots (PME is not built).
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._abi import TgnhError, _check


class DrudeForce:
    def __init__(self):
        self._particles = []         # [p, p1, p2, p3, p4, charge, polarizability, aniso12, aniso34]
        self._pairs = []             # [i, j, thole]

    # --- particles (OpenMM: DrudeForce::addParticle ...) ---
    def getNumParticles(self):
        return len(self._particles)

    def addParticle(self, particle, particle1, particle2, particle3, particle4, charge, polarizability, aniso12=0.0, aniso34=0.0):
        """A Drude particle `particle` on its parent `particle1`; particle2, and particle3 with particle4, name the anisotropy axes
        (-1: none).  Returns the row's index."""
        self._particles.append(self._row(particle, particle1, particle2, particle3, particle4, charge, polarizability, aniso12, aniso34))
        return len(self._particles) - 1

    def getParticleParameters(self, index):
        return tuple(self._particles[self._index(index, self._particles)])

    def setParticleParameters(self, index, particle, particle1, particle2, particle3, particle4, charge, polarizability, aniso12=0.0, aniso34=0.0):
        self._particles[self._index(index, self._particles)] = self._row(particle, particle1, particle2, particle3, particle4, charge,
                                                                         polarizability, aniso12, aniso34)

    # --- screened pairs (OpenMM: DrudeForce::addScreenedPair ...) ---
    def getNumScreenedPairs(self):
        return len(self._pairs)

    def addScreenedPair(self, particle1, particle2, thole):
        """Thole screening between the dipoles of rows `particle1` and `particle2` (indices as addParticle returned them)."""
        self._pairs.append([int(particle1), int(particle2), float(thole)])
        return len(self._pairs) - 1

    def getScreenedPairParameters(self, index):
        return tuple(self._pairs[self._index(index, self._pairs)])

    def setScreenedPairParameters(self, index, particle1, particle2, thole):
        self._pairs[self._index(index, self._pairs)] = [int(particle1), int(particle2), float(thole)]

    # --- the table as tgnh_set_drude_force takes it ---
    def tables(self):
        """-> (particles [n, 5] int32, params [n, 4] float64, screened [m, 2] int32, thole [m] float64)"""
        rows = np.array(self._particles, np.float64).reshape(-1, 9)
        pairs = np.array(self._pairs, np.float64).reshape(-1, 3)
        return (np.ascontiguousarray(rows[:, :5], np.int32), np.ascontiguousarray(rows[:, 5:]),
                np.ascontiguousarray(pairs[:, :2], np.int32), np.ascontiguousarray(pairs[:, 2]))

    @staticmethod
    def _row(p, p1, p2, p3, p4, charge, polarizability, aniso12, aniso34):
        return [int(p), int(p1), int(p2), int(p3), int(p4), float(charge), float(polarizability), float(aniso12), float(aniso34)]

    @staticmethod
    def _index(index, table):
        if not 0 <= index < len(table):                      # ASSERT_VALID_INDEX
            raise IndexError("Index out of range")
        return int(index)


class _TermTable:
    """Rows of `_WIDTH` particle indices, then `_EXTRA` integers, then two floats: the common part of the three bonded tables."""
    _WIDTH, _EXTRA = 0, 0

    def __init__(self):
        self._rows = []

    def _add(self, *row):
        self._rows.append(self._row(*row))
        return len(self._rows) - 1

    def _get(self, index):
        return tuple(self._rows[DrudeForce._index(index, self._rows)])

    def _set(self, index, *row):
        self._rows[DrudeForce._index(index, self._rows)] = self._row(*row)

    def _row(self, *row):
        ints = self._WIDTH + self._EXTRA
        if len(row) != ints + 2:
            raise TypeError(f"{type(self).__name__}: {ints + 2} values a row, got {len(row)}")
        return [int(v) for v in row[:ints]] + [float(v) for v in row[ints:]]

    def tables(self):
        """-> (particles [n, width] int32, params [n, 2] float64); a PeriodicTorsionForce: (particles [n, 4], periodicity [n] int32,
        params [n, 2] = (phase, k))"""
        w, x = self._WIDTH, self._EXTRA
        particles = np.ascontiguousarray([r[:w] for r in self._rows], np.int32).reshape(-1, w)
        params = np.ascontiguousarray([r[w + x:] for r in self._rows], np.float64).reshape(-1, 2)
        if not x:
            return particles, params
        return particles, np.ascontiguousarray([r[w] for r in self._rows], np.int32).reshape(-1), params


class HarmonicBondForce(_TermTable):
    """OpenMM's HarmonicBondForce as a table: E = 1/2 k (r - length)^2, length in nm, k in kJ/mol/nm^2."""
    _WIDTH = 2

    def getNumBonds(self):
        return len(self._rows)

    def addBond(self, particle1, particle2, length, k):
        return self._add(particle1, particle2, length, k)

    def getBondParameters(self, index):
        return self._get(index)

    def setBondParameters(self, index, particle1, particle2, length, k):
        self._set(index, particle1, particle2, length, k)


class HarmonicAngleForce(_TermTable):
    """OpenMM's HarmonicAngleForce as a table: E = 1/2 k (theta - angle)^2 about particle2, angle in rad, k in kJ/mol/rad^2."""
    _WIDTH = 3

    def getNumAngles(self):
        return len(self._rows)

    def addAngle(self, particle1, particle2, particle3, angle, k):
        return self._add(particle1, particle2, particle3, angle, k)

    def getAngleParameters(self, index):
        return self._get(index)

    def setAngleParameters(self, index, particle1, particle2, particle3, angle, k):
        self._set(index, particle1, particle2, particle3, angle, k)


class PeriodicTorsionForce(_TermTable):
    """OpenMM's PeriodicTorsionForce as a table: E = k (1 + cos(periodicity phi - phase)), phase in rad, k in kJ/mol."""
    _WIDTH, _EXTRA = 4, 1

    def getNumTorsions(self):
        return len(self._rows)

    def addTorsion(self, particle1, particle2, particle3, particle4, periodicity, phase, k):
        return self._add(particle1, particle2, particle3, particle4, periodicity, phase, k)

    def getTorsionParameters(self, index):
        return self._get(index)

    def setTorsionParameters(self, index, particle1, particle2, particle3, particle4, periodicity, phase, k):
        self._set(index, particle1, particle2, particle3, particle4, periodicity, phase, k)


class _ForceCallOut:
    """What BondedForces and NonbondedForces share: a force of the library's on `self.owner`'s handle that is computed into the owner's
    force buffer, gives its energy, and is a force call-out.  A subclass names its two library functions and its energy's width."""
    _COMPUTE = _ENERGY = None
    _ENERGY_WIDTH = 0

    def compute(self, energy=False):
        """tgnh_compute_*_force(s) on the owner's force buffer: the terms are ADDED to what it holds (nothing set: no launch).
        energy=True: the same launches leave the partial sums energy() adds.  No synchronisation."""
        o = self.owner
        force = getattr(o, "force", None)
        _check(getattr(o.lib, self._COMPUTE)(o.h, None if force is None else force.data_ptr(), 1 if energy else 0, o._stream()))

    def energy(self):
        """tgnh_get_*_energy: the class's components in kJ/mol, of the positions the last compute(energy=True) read.  Synchronises."""
        out = (C.c_double * self._ENERGY_WIDTH)()
        _check(getattr(self.owner.lib, self._ENERGY)(self.owner.h, self.owner._stream(), out))
        return tuple(float(e) for e in out)

    def __call__(self, ctx):
        """the form HipContext.force_fn takes"""
        ctx.force.zero_()
        self.compute()

    def then(self, fn):
        """-> a call-out that runs this one and then fn(ctx): for a caller who adds a force of their own behind it"""
        def both(ctx):
            self(ctx)
            fn(ctx)
        return both


class BondedForces(_ForceCallOut):
    """The library's bonded forces on a handle (include/drude_tgnh.h: tgnh_set_bonded_forces, ...).  `owner` is a HipContext or a
    HostTopology; bonds, angles, torsions: a HarmonicBondForce / HarmonicAngleForce / PeriodicTorsionForce, the tuple its tables()
    gives, or None.  Construction hands the tables to the handle (they replace the ones in force); a shape that does not fit is
    refused here, before any library call.  An instance is a force call-out: it zeroes the context's force buffer and adds the
    bonded forces, so `ctx.force_fn = BondedForces(ctx, ...)` is all a step, the minimiser or the barostat need.  energy():
    (bonds, angles, torsions)."""
    _COMPUTE, _ENERGY, _ENERGY_WIDTH = "tgnh_compute_bonded_forces", "tgnh_get_bonded_energy", 3

    def __init__(self, owner, bonds=None, angles=None, torsions=None):
        self.owner = owner
        b = self._tables("bonds", bonds, 2, False)
        a = self._tables("angles", angles, 3, False)
        t = self._tables("torsions", torsions, 4, True)
        ptr = lambda v, p: v.ctypes.data_as(p) if len(v) else None                                # noqa: E731
        _check(owner.lib.tgnh_set_bonded_forces(owner.h, len(b[0]), ptr(b[0], _lib.c_i32p), ptr(b[-1], _lib.c_f64p),
                                                len(a[0]), ptr(a[0], _lib.c_i32p), ptr(a[-1], _lib.c_f64p),
                                                len(t[0]), ptr(t[0], _lib.c_i32p), ptr(t[1], _lib.c_i32p), ptr(t[-1], _lib.c_f64p)))

    @staticmethod
    def _tables(name, table, width, periodic):
        """-> the table's arrays, contiguous and typed; TgnhError(ERR_ARG) for a shape that is not [n, width] beside [n, 2] (and [n])"""
        if table is None:
            table = (np.zeros((0, width), np.int32),) + ((np.zeros(0, np.int32),) if periodic else ()) + (np.zeros((0, 2)),)
        elif hasattr(table, "tables"):
            table = table.tables()
        if len(table) != (3 if periodic else 2):
            raise TgnhError(_lib.ERR_ARG, f"set_bonded_forces: {name}: {3 if periodic else 2} arrays, got {len(table)}")
        arrays = [np.ascontiguousarray(v, np.float64 if m == len(table) - 1 else np.int32) for m, v in enumerate(table)]
        n = len(arrays[0])
        if arrays[0].ndim != 2 or arrays[0].shape[1] != width:
            raise TgnhError(_lib.ERR_ARG, f"set_bonded_forces: {name}: particles of shape {arrays[0].shape}, not [n, {width}]")
        if arrays[-1].shape != (n, 2):
            raise TgnhError(_lib.ERR_ARG, f"set_bonded_forces: {name}: parameters of shape {arrays[-1].shape} for {n} rows of particles, not [{n}, 2]")
        if periodic and arrays[1].shape != (n,):
            raise TgnhError(_lib.ERR_ARG, f"set_bonded_forces: {name}: periodicities of shape {arrays[1].shape} for {n} rows of particles, not [{n}]")
        return arrays

    @property
    def num_terms(self):
        """tgnh_get_num_bonded_terms: (bonds, angles, torsions) of the tables in force"""
        out = (C.c_int * 3)()
        _check(self.owner.lib.tgnh_get_num_bonded_terms(self.owner.h, out))
        return tuple(out)

    def clear(self):
        """all three counts 0: the tables are gone, compute() launches nothing"""
        _check(self.owner.lib.tgnh_set_bonded_forces(self.owner.h, 0, None, None, 0, None, None, 0, None, None, None))


class _NonbondedDesc(C.Structure):
    """tgnh_nonbonded_desc (tgnh_set_nonbonded_force)"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("method", C.c_int32), ("cutoff", C.c_double), ("reaction_field_dielectric", C.c_double),
        ("num_particles", C.c_int32), ("particles", C.c_void_p), ("num_exceptions", C.c_int32), ("exception_particles", C.c_void_p),
        ("exception_params", C.c_void_p),
    ]


class NonbondedForce:
    """OpenMM's NonbondedForce as a table: per particle (charge e, sigma nm, epsilon kJ/mol), exceptions (p1, p2, chargeProd, sigma,
    epsilon), the method, the cutoff and the reaction field's dielectric.  The library takes CutoffPeriodic, and Ewald through
    NonbondedForces (the other methods are refused by tgnh_set_nonbonded_force, not here)."""
    NoCutoff, CutoffNonPeriodic, CutoffPeriodic, Ewald = 0, 1, 2, 3      # OpenMM's numbering

    def __init__(self):
        self._particles = []         # [charge, sigma, epsilon]
        self._exceptions = []        # [p1, p2, chargeProd, sigma, epsilon]
        self._pair_index = {}        # (lo, hi) -> row of _exceptions
        self._method = self.NoCutoff                             # OpenMM's defaults
        self._cutoff = 1.0
        self._dielectric = 78.3
        self._ewald_tolerance = 5e-4
        self._ewald = (0.0, 0, 0, 0)                             # alpha, kmaxx, kmaxy, kmaxz; all zero: derived from the tolerance
        self._pme = (0.0, 0, 0, 0)                               # alpha, nx, ny, nz; all zero: derived from the tolerance

    # --- particles ---
    def getNumParticles(self):
        return len(self._particles)

    def addParticle(self, charge, sigma, epsilon):
        self._particles.append([float(charge), float(sigma), float(epsilon)])
        return len(self._particles) - 1

    def getParticleParameters(self, index):
        return tuple(self._particles[DrudeForce._index(index, self._particles)])

    def setParticleParameters(self, index, charge, sigma, epsilon):
        self._particles[DrudeForce._index(index, self._particles)] = [float(charge), float(sigma), float(epsilon)]

    # --- exceptions ---
    def getNumExceptions(self):
        return len(self._exceptions)

    def addException(self, particle1, particle2, chargeProd, sigma, epsilon, replace=False):
        """A pair left out of the nonbonded loop and, unless chargeProd and epsilon are both 0, evaluated with these parameters.  A
        pair that already has an exception: ValueError, or with replace=True its row is overwritten.  Returns the row's index."""
        p1, p2 = int(particle1), int(particle2)
        key = (min(p1, p2), max(p1, p2))
        row = [p1, p2, float(chargeProd), float(sigma), float(epsilon)]
        if key in self._pair_index:
            if not replace:
                raise ValueError(f"NonbondedForce: There is already an exception for particles {p1} and {p2}")
            self._exceptions[self._pair_index[key]] = row
            return self._pair_index[key]
        self._exceptions.append(row)
        self._pair_index[key] = len(self._exceptions) - 1
        return len(self._exceptions) - 1

    def getExceptionParameters(self, index):
        return tuple(self._exceptions[DrudeForce._index(index, self._exceptions)])

    def setExceptionParameters(self, index, particle1, particle2, chargeProd, sigma, epsilon):
        index = DrudeForce._index(index, self._exceptions)
        old = self._exceptions[index]
        p1, p2 = int(particle1), int(particle2)
        key = (min(p1, p2), max(p1, p2))
        if self._pair_index.get(key, index) != index:
            raise ValueError(f"NonbondedForce: There is already an exception for particles {p1} and {p2}")
        del self._pair_index[(min(old[0], old[1]), max(old[0], old[1]))]
        self._pair_index[key] = index
        self._exceptions[index] = [p1, p2, float(chargeProd), float(sigma), float(epsilon)]

    def createExceptionsFromBonds(self, bonds, coulomb14Scale, lj14Scale):
        """OpenMM's rule: particles one or two bonds apart become pure exclusions; particles three bonds apart (and no closer by
        another path) get chargeProd = coulomb14Scale q_i q_j, the mean sigma and epsilon = lj14Scale sqrt(eps_i eps_j).  Pairs that
        already have an exception keep it."""
        n = len(self._particles)
        near = [set() for _ in range(n)]
        for a, b in bonds:
            a, b = int(a), int(b)
            if not (0 <= a < n and 0 <= b < n):
                raise IndexError("createExceptionsFromBonds: Illegal particle index in list of bonds")
            near[a].add(b); near[b].add(a)
        for i in range(n):
            one = near[i]
            two = set().union(*(near[j] for j in one)) - one - {i} if one else set()
            three = (set().union(*(near[j] for j in two)) if two else set()) - two - one - {i}
            for j in sorted(one | two):
                if j > i and (i, j) not in self._pair_index:
                    self.addException(i, j, 0.0, 1.0, 0.0)
            for j in sorted(three):
                if j > i and (i, j) not in self._pair_index:
                    (qi, si, ei), (qj, sj, ej) = self._particles[i], self._particles[j]
                    self.addException(i, j, coulomb14Scale * qi * qj, 0.5 * (si + sj), lj14Scale * (ei * ej) ** 0.5)

    # --- the method and its parameters ---
    def getNonbondedMethod(self):
        return self._method

    def setNonbondedMethod(self, method):
        if method not in (self.NoCutoff, self.CutoffNonPeriodic, self.CutoffPeriodic, self.Ewald):
            raise ValueError("NonbondedForce: Illegal value for nonbonded method")
        self._method = int(method)

    def getCutoffDistance(self):
        return self._cutoff

    def setCutoffDistance(self, distance):
        self._cutoff = float(distance)

    def getReactionFieldDielectric(self):
        return self._dielectric

    def setReactionFieldDielectric(self, dielectric):
        self._dielectric = float(dielectric)

    # --- Ewald summation ---
    def getEwaldErrorTolerance(self):
        return self._ewald_tolerance

    def setEwaldErrorTolerance(self, tol):
        self._ewald_tolerance = float(tol)

    def getEwaldParameters(self):
        return self._ewald

    def setEwaldParameters(self, alpha, kmaxx, kmaxy, kmaxz):
        """alpha (nm^-1) and the largest reciprocal index per axis; all zero: ewald_parameters derives them from the tolerance"""
        self._ewald = (float(alpha), int(kmaxx), int(kmaxy), int(kmaxz))

    def ewald_parameters(self, box):
        """-> (alpha, kmaxx, kmaxy, kmaxz) for a box given as three edges or three vectors (nm): what setEwaldParameters holds, or,
        where that is all zero, OpenMM's rule from the error tolerance and the cutoff as recalled (OpenMM was not at hand to check
        against): alpha = sqrt(-ln(2 tol)) / rc, and kmax_d the smallest k >= 1 with
        k sqrt(L_d alpha) / 20 exp(-(pi k / (L_d alpha))^2) <= tol.  The rule is a heuristic, not a bound."""
        if self._ewald != (0.0, 0, 0, 0):
            return self._ewald
        box = np.asarray(box, np.float64)
        edges = np.diag(box) if box.ndim == 2 else box
        tol = self._ewald_tolerance
        alpha = math.sqrt(-math.log(2.0 * tol)) / self._cutoff
        kmax = []
        for edge in edges:
            k = 1
            while k * math.sqrt(edge * alpha) / 20.0 * math.exp(-(math.pi * k / (edge * alpha)) ** 2) > tol:
                k += 1
            kmax.append(k)
        return (alpha, kmax[0], kmax[1], kmax[2])

    # --- particle-mesh Ewald ---
    def getPMEParameters(self):
        return self._pme

    def setPMEParameters(self, alpha, nx, ny, nz):
        """alpha (nm^-1) and the grid; all zero: pme_parameters derives them from the tolerance"""
        self._pme = (float(alpha), int(nx), int(ny), int(nz))

    def pme_parameters(self, box):
        """-> (alpha, nx, ny, nz) for a box given as three edges or three vectors (nm): what setPMEParameters holds, or, where that
        is all zero, OpenMM's rule from the error tolerance and the cutoff as recalled (OpenMM was not at hand to check against):
        alpha = sqrt(-ln(2 tol)) / rc, and N_d = ceil(2 alpha L_d / (3 tol^(1/5))), at least 6, raised to the next size whose prime
        factors are 2, 3 and 5 only.  The rule is a heuristic, not a bound."""
        if self._pme != (0.0, 0, 0, 0):
            return self._pme
        box = np.asarray(box, np.float64)
        edges = np.diag(box) if box.ndim == 2 else box
        tol = self._ewald_tolerance
        alpha = math.sqrt(-math.log(2.0 * tol)) / self._cutoff
        grid = []
        for edge in edges:
            n = max(6, int(math.ceil(2.0 * alpha * edge / (3.0 * tol ** 0.2))))
            while not self._smooth(n):
                n += 1
            grid.append(n)
        return (alpha, grid[0], grid[1], grid[2])

    @staticmethod
    def _smooth(n):
        for r in (2, 3, 5):
            while n % r == 0:
                n //= r
        return n == 1

    # --- the table as tgnh_set_nonbonded_force takes it ---
    def tables(self):
        """-> (method, cutoff, dielectric, particles [n, 3] float64, exception_particles [ne, 2] int32, exception_params [ne, 3] float64)"""
        exc = np.array(self._exceptions, np.float64).reshape(-1, 5)
        return (self._method, self._cutoff, self._dielectric, np.array(self._particles, np.float64).reshape(-1, 3),
                np.ascontiguousarray(exc[:, :2], np.int32), np.ascontiguousarray(exc[:, 2:]))


class NonbondedForces(_ForceCallOut):
    """The library's NonbondedForce on a handle (include/drude_tgnh.h: tgnh_set_nonbonded_force, ...).  `owner` is a HipContext or a
    HostTopology; `force` a NonbondedForce, the tuple its tables() gives, or None (nothing set).  Construction hands the table to
    the handle (it replaces the one in force); a shape that does not fit is refused here, before any library call.  The box is the
    handle's (setPeriodicBoxVectors).  An instance is a force call-out, and `BondedForces(ctx, ...).then(lambda c: nb.compute())`
    adds it behind the bonded forces.  energy(): (pair Coulomb with the reaction field, pair Lennard-Jones, exception Coulomb,
    exception Lennard-Jones).

    Ewald summation (tgnh_set_nonbonded_ewald): a NonbondedForce whose method is Ewald is handed over as CutoffPeriodic and Ewald is
    switched on behind it, with `ewald` = (alpha, kmaxx, kmaxy, kmaxz) if given, otherwise force.ewald_parameters(the owner's box) --
    an owner without a box is refused with ERR_STATE before any library call.  `ewald` beside a CutoffPeriodic table switches it on
    as well; a raw tuple whose method is 3 is refused by the library as before.  `ewald`: (alpha, (kx, ky, kz), M) or None;
    ewald_energy(): (reciprocal, self, neutralising background, exclusion correction); energy()[0] is then the direct-space sum.

    Particle-mesh Ewald (tgnh_set_nonbonded_pme), the other form of the same setting: `pme` = (alpha, nx, ny, nz) switches it on
    behind the table, whether the table's method is CutoffPeriodic or Ewald; `pme=True` takes force.pme_parameters(the owner's box)
    -- an owner without a box is refused with ERR_STATE before any library call.  `ewald` and `pme` together: ERR_ARG.  `pme`:
    (alpha, (nx, ny, nz)) or None; with it in force `ewald` is None and ewald_energy()[0] is the mesh sum; pme_grids(): the last
    call's charge grid (int64, x 2^48) and potential, [nz, ny, nx]."""
    _COMPUTE, _ENERGY, _ENERGY_WIDTH = "tgnh_compute_nonbonded_force", "tgnh_get_nonbonded_energy", 4

    def __init__(self, owner, force=None, ewald=None, pme=None):
        self.owner = owner
        if force is None:
            self.clear()
            return
        if ewald is not None and pme is not None:
            raise TgnhError(_lib.ERR_ARG, "set_nonbonded_force: ewald= and pme= are two forms of one setting: pass one of them")
        table = force.tables() if hasattr(force, "tables") else force
        if pme is True:
            if not hasattr(force, "pme_parameters"):
                raise TgnhError(_lib.ERR_ARG, "set_nonbonded_force: pme=True takes the parameters from a NonbondedForce; beside a tuple pass pme=(alpha, nx, ny, nz)")
            box = owner.getPeriodicBoxVectors()
            if box is None:
                raise TgnhError(_lib.ERR_STATE, "set_nonbonded_force: the PME parameters come from the box, and the owner has none: "
                                                "call setPeriodicBoxVectors first, or pass pme=(alpha, nx, ny, nz)")
            pme = force.pme_parameters(box)
        if pme is not None:
            pme = tuple(pme)
            if len(pme) != 4:
                raise TgnhError(_lib.ERR_ARG, f"set_nonbonded_force: pme: (alpha, nx, ny, nz), got {len(pme)} values")
        if hasattr(force, "tables") and len(table) == 6 and int(table[0]) == NonbondedForce.Ewald:
            if ewald is None and pme is None:
                box = owner.getPeriodicBoxVectors()
                if box is None:
                    raise TgnhError(_lib.ERR_STATE, "set_nonbonded_force: the Ewald parameters come from the box, and the owner has none: "
                                                    "call setPeriodicBoxVectors first, or pass ewald=(alpha, kmaxx, kmaxy, kmaxz)")
                ewald = force.ewald_parameters(box)
            table = (NonbondedForce.CutoffPeriodic,) + tuple(table[1:])
        if ewald is not None:
            ewald = tuple(ewald)
            if len(ewald) != 4:
                raise TgnhError(_lib.ERR_ARG, f"set_nonbonded_force: ewald: (alpha, kmaxx, kmaxy, kmaxz), got {len(ewald)} values")
        if len(table) != 6:
            raise TgnhError(_lib.ERR_ARG, f"set_nonbonded_force: a method, a cutoff, a dielectric and three arrays, got {len(table)} values")
        method, cutoff, dielectric = int(table[0]), float(table[1]), float(table[2])
        par, ep, ex = (np.ascontiguousarray(v, t) for v, t in zip(table[3:], (np.float64, np.int32, np.float64)))
        if par.ndim != 2 or par.shape[1] != 3:
            raise TgnhError(_lib.ERR_ARG, f"set_nonbonded_force: particles of shape {par.shape}, not [n, 3]")
        ne = len(ep)
        if ep.shape != (ne, 2):
            raise TgnhError(_lib.ERR_ARG, f"set_nonbonded_force: exception particles of shape {ep.shape}, not [ne, 2]")
        if ex.shape != (ne, 3):
            raise TgnhError(_lib.ERR_ARG, f"set_nonbonded_force: exception parameters of shape {ex.shape} for {ne} rows of particles, not [{ne}, 3]")
        d = _NonbondedDesc(C.sizeof(_NonbondedDesc), method, cutoff, dielectric, len(par), par.ctypes.data if len(par) else None,
                           ne, ep.ctypes.data if ne else None, ex.ctypes.data if ne else None)
        _check(owner.lib.tgnh_set_nonbonded_force(owner.h, C.byref(d)))
        if ewald is not None:
            self.set_ewald(*ewald)
        if pme is not None:
            self.set_pme(*pme)

    def set_pme(self, alpha, nx, ny, nz):
        """tgnh_set_nonbonded_pme on the table in force"""
        e = _lib.TgnhPmeDesc(C.sizeof(_lib.TgnhPmeDesc), (C.c_int32 * 3)(int(nx), int(ny), int(nz)), float(alpha))
        _check(self.owner.lib.tgnh_set_nonbonded_pme(self.owner.h, C.byref(e)))

    def clear_pme(self):
        """back to the reaction field"""
        _check(self.owner.lib.tgnh_set_nonbonded_pme(self.owner.h, None))

    @property
    def pme(self):
        """tgnh_get_nonbonded_pme: (alpha, (nx, ny, nz)) of the setting in force, None: off"""
        e = _lib.TgnhPmeDesc()
        _check(self.owner.lib.tgnh_get_nonbonded_pme(self.owner.h, C.byref(e)))
        return (float(e.alpha), tuple(e.grid)) if e.struct_size else None

    def pme_grids(self):
        """tgnh_get_pme_grids: (charge int64 [nz, ny, nx], the spread charges x 2^48; potential float64 [nz, ny, nx]) of the last
        compute().  Synchronises."""
        setting = self.pme
        if setting is None:
            _check(self.owner.lib.tgnh_get_pme_grids(self.owner.h, self.owner._stream(), None, None))
        nx, ny, nz = setting[1]
        charge, potential = np.empty((nz, ny, nx), np.int64), np.empty((nz, ny, nx), np.float64)
        _check(self.owner.lib.tgnh_get_pme_grids(self.owner.h, self.owner._stream(), charge.ctypes.data, potential.ctypes.data))
        return charge, potential

    def set_ewald(self, alpha, kmaxx, kmaxy, kmaxz):
        """tgnh_set_nonbonded_ewald on the table in force"""
        e = _lib.TgnhEwaldDesc(C.sizeof(_lib.TgnhEwaldDesc), (C.c_int32 * 3)(int(kmaxx), int(kmaxy), int(kmaxz)), float(alpha))
        _check(self.owner.lib.tgnh_set_nonbonded_ewald(self.owner.h, C.byref(e)))

    def clear_ewald(self):
        """back to the reaction field"""
        _check(self.owner.lib.tgnh_set_nonbonded_ewald(self.owner.h, None))

    @property
    def ewald(self):
        """tgnh_get_nonbonded_ewald: (alpha, (kmaxx, kmaxy, kmaxz), M reciprocal vectors) of the setting in force, None: off"""
        e, m = _lib.TgnhEwaldDesc(), C.c_int(0)
        _check(self.owner.lib.tgnh_get_nonbonded_ewald(self.owner.h, C.byref(e), C.byref(m)))
        return (float(e.alpha), tuple(e.kmax), int(m.value)) if e.struct_size else None

    def ewald_energy(self):
        """tgnh_get_ewald_energy: (reciprocal, self, neutralising background, exclusion correction) in kJ/mol, of the positions the
        last compute(energy=True) read.  Synchronises."""
        out = (C.c_double * 4)()
        _check(self.owner.lib.tgnh_get_ewald_energy(self.owner.h, self.owner._stream(), out))
        return tuple(float(v) for v in out)

    @property
    def num_terms(self):
        """tgnh_get_num_nonbonded_terms: (particles, exceptions, of which evaluated) of the table in force"""
        out = (C.c_int * 3)()
        _check(self.owner.lib.tgnh_get_num_nonbonded_terms(self.owner.h, out))
        return tuple(out)

    def clear(self):
        """the table is gone, compute() launches nothing"""
        _check(self.owner.lib.tgnh_set_nonbonded_force(self.owner.h, None))
