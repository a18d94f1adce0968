"""The feature units of include/drude_tgnh.h, one short section each: centre-of-mass motion, velocity rescaling, the velocity draw,
the barostat's trial move, wrap and frames, the minimiser, the direct constraint solver, virtual sites, DrudeForce and the Drude
statistics.  Their tables live on the handle (handle.py); here are the launches.  A call that writes velocities ends in
`_wrote_velocities` (stepping.py)."""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import TgnhError, _check, f64
from .handle import Handle
from .records import DrudeStatistics, Momentum, MinimizeState, minimize_desc


class Features(Handle):
    # ---- centre-of-mass motion (include/drude_tgnh.h: tgnh_get_momentum, tgnh_remove_cm_motion, ...) ----
    def momentum(self):
        """tgnh_get_momentum: total mass and momentum of this context's slots, summed on the device (what a step left owed to the
        velocities is applied first).  Synchronises the stream.  In a sharded run every context answers for its own slots; the
        fields add up over ranks."""
        st = _lib.TgnhMomentum(struct_size=C.sizeof(_lib.TgnhMomentum))
        _check(self.lib.tgnh_get_momentum(self.h, self._stream(), C.byref(st)))
        return Momentum(st)

    def removeCMMotion(self):
        """tgnh_remove_cm_motion: v -= P / M on every massive slot, on the device and without a host synchronisation; with an
        all-reduce set (set_allreduce, rccl_init) P and M are the whole system's, and the call is collective."""
        self._wrote_velocities(self.lib.tgnh_remove_cm_motion(self.h, self._stream()))

    def shift_velocities(self, dv):
        """tgnh_shift_velocities: v -= dv on every massive slot."""
        p = f64(dv, (3,), "shift_velocities", "dv must have three components")[1]
        self._wrote_velocities(self.lib.tgnh_shift_velocities(self.h, p, self._stream()))

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
        f, p = f64(factors)
        if f.ndim != 1:
            raise TgnhError(_lib.ERR_ARG, "scale_velocities: factors must be a vector, one per thermostat")
        self._wrote_velocities(self.lib.tgnh_scale_velocities(self.h, p, len(f), self._stream()))

    def rescale_to_temperature(self, temperature=None, drudeTemperature=None):
        """tgnh_rescale_to_temperature: every thermostat's kinetic energy onto N kT at these temperatures (default: the
        integrator's) -- kinetic-energy pass, all-reduce where one is set (the call is then collective), factors, rescale, all on
        the device.  The baths stay as they are.  last_kinetic_energies() has the sums before scaling, rescale_factors() the
        factors."""
        self._wrote_velocities(self.lib.tgnh_rescale_to_temperature(self.h, *self._bath_pair(temperature, drudeTemperature), self._stream()))

    def rescale_factors(self):
        """tgnh_get_rescale_factors: what the last scale_velocities / rescale_to_temperature applied.  Synchronises the stream."""
        return self._vec(self.lib.tgnh_get_rescale_factors, self.num_thermostats())

    def set_velocity_rescaling(self, every, temperature=None, drudeTemperature=None):
        """tgnh_set_velocity_rescaling: rescale_to_temperature before every step whose number is a multiple of `every` (0: off),
        after a centre-of-mass removal due at the same step, inside step() and whatever else runs the step entry points."""
        _check(self.lib.tgnh_set_velocity_rescaling(self.h, int(every), *self._bath_pair(temperature, drudeTemperature)))
        self.velocity_rescaling = int(every)
        self._wrote_velocities()

    # ---- the velocity draw (include/drude_tgnh.h: tgnh_set_velocities_to_temperature) ----
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
        self._wrote_velocities(self.lib.tgnh_set_velocities_to_temperature(self.h, float(temperature), float(drudeTemperature), seed,
                                                                           int(self.first_particle), self._stream()))
        if self._has_clusters:
            _check(self.lib.tgnh_harness_shake_velocities(self.h, self.integrator.getConstraintTolerance(), self._stream()))
            _check(self.lib.tgnh_apply_velocity_constraints(self.h, self.integrator.getConstraintTolerance(), self._stream()))
        if removeCMMotion:
            self.removeCMMotion()
        if exact:
            self.rescale_to_temperature(temperature, drudeTemperature)

    # ---- the barostat's trial move (include/drude_tgnh.h: tgnh_scale_positions, tgnh_restore_positions) ----
    def scale_positions(self, scale, save=False):
        """tgnh_scale_positions: every molecule of the table in force (set_molecules) moved rigidly by (scale - 1) x its centroid,
        about the origin; a scalar means isotropic.  save=True keeps what was read in a snapshot of the handle's
        (restore_positions), in the same launch.  No host synchronisation; velocities, thermostat and everything a step left
        pending stay as they are.  Refused while a half kick is owed to the velocities (flush() first).  The caller scales its own
        box and recomputes the forces before the next step."""
        p = f64(np.broadcast_to(np.asarray(scale, np.float64), (3,)) if np.ndim(scale) == 0 else scale, (3,),
                "scale_positions", "scale is a scalar or has three components")[1]
        _check(self.lib.tgnh_scale_positions(self.h, p, int(bool(save)), self._stream()))

    def restore_positions(self):
        """tgnh_restore_positions: the positions (and charges) as the last scale_positions(save=True) read them, bit for bit."""
        _check(self.lib.tgnh_restore_positions(self.h, self._stream()))

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
        d = _lib.TgnhFrameDesc(struct_size=C.sizeof(_lib.TgnhFrameDesc))
        d.flags = (_lib.FRAME_WRAP if wrap else 0) | (_lib.FRAME_SKIP_DRUDE if skip_drude else 0) | (0 if planes else _lib.FRAME_INTERLEAVED)
        d.unit, d.stride, d.capacity = float(unit), count if planes else 0, 3 * count
        _check(self.lib.tgnh_write_frame(self.h, C.byref(d), out.data_ptr(), self._stream()))
        return out

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
        if self._c_loops_can_run() and not sites:            # (and no sites: the minimiser's C loop places none)
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
        call-out and, with site_forces set, their forces spread after it, so every massive slot may move.  Velocities, thermostat
        and step count stay as they are.  Returns a MinimizeState; unless it says converged == 1 the forces are recomputed at the
        final positions."""
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

    # ---- the direct constraint solver (include/drude_tgnh.h: tgnh_apply_constraints, tgnh_apply_velocity_constraints) ----
    @property
    def constraint_clusters(self):
        """(direct, harness): the clusters in the direct solver's table and in the harness' SHAKE table"""
        return self.num_constraint_clusters(), self._harness_clusters

    def _tol(self, tol):
        return self.integrator.getConstraintTolerance() if tol is None else float(tol)

    def apply_constraints(self, tol=None):
        """tgnh_apply_constraints: the direct solver on posDelta, for the clusters of its table (tol=None: the integrator's
        constraint tolerance; it gates the result, status bit 1, and does not steer the solve).  No synchronisation."""
        _check(self.lib.tgnh_apply_constraints(self.h, self._tol(tol), self._stream()))

    def apply_velocity_constraints(self, tol=None):
        """tgnh_apply_velocity_constraints: the direct solver's velocity stage on velm (one linear solve per cluster)."""
        self._wrote_velocities(self.lib.tgnh_apply_velocity_constraints(self.h, self._tol(tol), self._stream()))

    # ---- the library's own virtual-site stage (include/drude_tgnh.h: tgnh_set_virtual_sites, ...) ----
    def set_virtual_sites(self, kinds, atoms, params):
        """tgnh_set_virtual_sites (see Handle.set_virtual_sites); a context with sites steps along the split path, the one with the
        virtual-site call-out."""
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
        return tuple(float(e) for e in self._vec(self.lib.tgnh_get_drude_energy, 2))

    # ---- Drude pair statistics (include/drude_tgnh.h: tgnh_get_drude_statistics) ----
    def drude_statistics(self, threshold=None, hist_max=0.0):
        """tgnh_get_drude_statistics: the Drude-parent distances and the induced dipole of the positions as they are, summed on
        the device (no copy of the positions, no flush).  threshold=None: the integrator's getMaxDrudeDistance().  Synchronises
        the stream.  In a sharded run every context answers for its own slots (see include/drude_tgnh.h for what adds up)."""
        if threshold is None:
            threshold = self.integrator.getMaxDrudeDistance()
        st = _lib.TgnhDrudeStats(struct_size=C.sizeof(_lib.TgnhDrudeStats))
        _check(self.lib.tgnh_get_drude_statistics(self.h, float(threshold), float(hist_max), self._stream(), C.byref(st)))
        return DrudeStatistics(st, float(threshold), float(hist_max))
