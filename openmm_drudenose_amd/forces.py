"""Forces the library computes itself, for a host that has no OpenMM behind it.

`DrudeForce` keeps the method names and argument order of OpenMM's DrudeForce (addParticle / addScreenedPair and their getters and
setters); it holds the table only.  `tables()` gives it in the form tgnh_set_drude_force takes (include/drude_tgnh.h has the
contract and the terms); `DrudeSystem.set_drude_force` attaches it to a system, and a `HipContext` over such a system hands it to
its handle.  Units are OpenMM's: charge e, polarizability nm^3.
"""
import numpy as np


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
