"""`DrudeTGNHIntegrator`: the mirror of the reference's Python class.  It keeps the method names, argument meaning, defaults and error
behaviour of the SWIG class (python/drudetgnhplugin.i:60-92 of scychon/openmm_drudeNose, C++ side
openmmapi/src/DrudeTGNHIntegrator.cpp).  No ctypes here: a bound integrator talks to its context, the context to the library."""
import numpy as np

from . import _lib
from ._abi import TgnhError


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
    def setTemperature(self, temp): self._set_bath("_temperature", temp)
    def getCouplingTime(self): return self._couplingTime
    def setCouplingTime(self, tau): self._couplingTime = float(tau)
    def getDrudeTemperature(self): return self._drudeTemperature
    def setDrudeTemperature(self, temp): self._set_bath("_drudeTemperature", temp)

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
