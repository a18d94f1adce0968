"""Taking time steps (include/drude_tgnh.h: tgnh_step_*, tgnh_run_*, tgnh_flush, tgnh_get_pending_state, ...): the force call-out,
the step entry points, step() and its choice between the library's C loops and the Python loop, steps captured into a hipGraph,
and what a step leaves behind -- pending state, velocity planes, status word, kinetic energies, clock and timing.

The cached kinetic-energy sum (`ke_sum_valid`, DrudeTGNHIntegrator.cpp:166-170, :192) is touched in two places only:
`_wrote_velocities` clears it and `_stepped` sets it.  Every call of any part that writes velocities goes through the first."""
import ctypes as C

from . import _lib
from ._abi import TgnhError, _check
from .handle import Handle


class Stepping(Handle):
    # ---- the two markers of the cached kinetic-energy sum ----
    def _wrote_velocities(self, rc=_lib.TGNH_OK):
        """this call wrote velocities: the cached sum is stale (a refused call raises and leaves it)"""
        _check(rc)
        self.ke_sum_valid = False

    def _stepped(self, rc=_lib.TGNH_OK, steps=1):
        """`steps` finished steps: the last one left its sum (DrudeTGNHIntegrator.cpp:192); none: as it was"""
        _check(rc)
        if steps > 0:
            self.ke_sum_valid = True

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

    # ---- the call-outs of a step ----
    def compute_forces(self):
        if self.force_fn is not None:
            self.force_fn(self)
        else:
            _check(self.lib.tgnh_harness_force(self.h, self._x0_arg(), self.k_drude, self.k_tether, self.force.data_ptr(), self._stream()))
        if self.drude_force:
            self.compute_drude_force()
        if self.site_forces:
            self.distribute_site_forces()

    def _place_sites(self):
        """the virtual-site call-out (Cu :377): the harness' table where it holds sites, then the library's (none: no launch)"""
        if self._harness_sites:
            _check(self.lib.tgnh_harness_virtual_sites(self.h, self._stream()))
        _check(self.lib.tgnh_compute_virtual_sites(self.h, self._stream()))

    # ---- which loop runs the steps ----
    def _c_loops_can_run(self):
        """The library's C loops know the harness force alone: they can run this context's call-outs when there is no force_fn of
        the caller's and no DrudeForce stage.  A stage the loops do not know is added here, once."""
        return self.force_fn is None and not self.drude_force

    def _c_loop(self, steps, forces=True):
        """Enqueues `steps` steps with the C loop for this context -> its status: the split entry points around the harness'
        constraint and virtual-site call-outs for a constrained one, else the harness force between step_begin and step_end, or
        (forces=False) nothing between them.  Callers refuse forces=False on a constrained context; a finished run is `_stepped`."""
        if self.constrained:
            return self.lib.tgnh_run_harness_constrained(self.h, self._x0_arg(), self.k_drude, self.k_tether,
                                                         self.integrator.getConstraintTolerance(), int(steps), self._stream())
        if not forces:
            return self.lib.tgnh_run_steps(self.h, int(steps), self._stream())
        return self.lib.tgnh_run_harness(self.h, self._x0_arg(), self.k_drude, self.k_tether, int(steps), self._stream())

    def step_begin(self): _check(self.lib.tgnh_step_begin(self.h, self._stream()))

    def step_end(self): self._stepped(self.lib.tgnh_step_end(self.h, self._stream()))

    def step(self, steps):
        if self._c_loops_can_run():
            return self._stepped(self._c_loop(steps), steps)
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
            if self.mode == _lib.MODE_TGNH:
                _check(lib.tgnh_harness_shake_velocities(h, tol, self._stream()))   # Cu :391
                _check(lib.tgnh_apply_velocity_constraints(h, tol, self._stream()))
            self._stepped(lib.tgnh_step_end_thermo(h, self._stream()))   # Cu :394-406

    def step_without_forces(self, steps):
        """`steps` x (step_begin, step_end) with NO force call-out, on whatever the force buffer holds: for timing the integrator's
        own launches (bench.py's integrator_only leg); not a trajectory of anything."""
        if self.constrained:
            raise TgnhError(_lib.ERR_STATE, "step_without_forces: unconstrained systems only")
        self._stepped(self._c_loop(steps, forces=False), steps)

    def capture_steps(self, steps, forces=True):
        """Captures `steps` time steps (harness force call-out included -- and the harness' constraint / virtual-site call-outs for a
        system with constraints --, and the KE all-reduce when sharded; forces=False: no call-out, see step_without_forces) into
        a hipGraph on a side stream and returns a callable that replays it.  The step sequence must not change afterwards
        (no setters).  A handle that is not in the steady state of its step sequence is brought there first, by up to
        three times `steps` real steps (see below): read the step count afterwards if it matters."""
        torch = self.torch
        # every refusal stands in front of the first capture: nothing raises through an open one
        if not self._c_loops_can_run():
            raise TgnhError(_lib.ERR_STATE, "capture_steps supports the harness force call-out only")
        # A recording bakes in the centre-of-mass removals of the steps it recorded (set_cm_motion_removal): it replays the loop's
        # own launches only if every replay starts at a multiple of the interval, and so ends at one
        # (and the velocity rescalings, set_velocity_rescaling, alike)
        for what, every in (("centre-of-mass removal", self.cm_motion_removal), ("velocity rescaling", self.velocity_rescaling)):
            if every > 0 and (self.time()[1] % every or int(steps) % every):
                raise TgnhError(_lib.ERR_STATE, f"capture_steps: with {what} every {every} steps, the step count at the "
                                f"capture ({self.time()[1]}) and the steps captured ({int(steps)}) must both be multiples of it")
        if self.constrained and not forces:
            raise TgnhError(_lib.ERR_STATE, "capture_steps(forces=False): unconstrained systems only")
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
                _check(self._c_loop(steps, forces))          # the step loop step() runs for such a system; recorded, not run
            return g
        for _ in range(4):
            owed_before = self.pending_state() & _lib.PENDING_OWED
            first = record()
            if self.pending_state() & _lib.PENDING_OWED == owed_before:
                break
            first.replay()                                   # a transition: taken for real (the recording has advanced the clock)
            torch.cuda.synchronize(self.dev)
            self._stepped()
        else:
            raise TgnhError(_lib.ERR_STATE, "capture_steps: the handle does not reach a steady state of its step sequence")
        clock = self.time()
        graphs = [first, record()]
        if self.pending_state() & _lib.PENDING_OWED != owed_before:
            raise TgnhError(_lib.ERR_STATE, "capture_steps: the step sequence is not periodic")
        # a capture advances the host-side clock without running anything: the first one stands for the first replay,
        # the second one is taken back
        self.set_time(*clock)
        self._captured_not_run = int(steps)
        turn = [0]
        baths = self._bath_epoch
        planes = owed_before & _lib.PENDING_VELOCITY_PLANES

        def replay():
            # the launches of a recording read the velocities where they lived when it was made (the one-launch step's own planes,
            # or velm): a query or a flush since has moved them, and a replay would step from stale ones
            if (self.pending_state() ^ planes) & _lib.PENDING_VELOCITY_PLANES:
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
            self._stepped()
        replay.graph, replay.graphs = graphs[0], graphs
        return replay

    # ---- what a step leaves behind ----
    def flush(self):
        """velm <- the reference's end-of-step velocities (a deferred variant's pending half kick and factors applied)"""
        _check(self.lib.tgnh_flush(self.h, self._stream()))

    def pending_state(self):
        """tgnh_get_pending_state: what the handle still owes the trajectory (bit set, include/drude_tgnh.h; _lib.PENDING_*)."""
        return self._get(self.lib.tgnh_get_pending_state, C.c_uint32)

    def velocity_planes(self):
        """tgnh_get_velocity_planes: (live, usable, one-launch steps in a row since the last settle, the threshold) -- whether the
        one-launch step keeps the velocities in its own x | y | z planes right now, and whether this handle ever can."""
        out = (C.c_int32 * 4)()
        _check(self.lib.tgnh_get_velocity_planes(self.h, out))
        return bool(out[0]), bool(out[1]), int(out[2]), int(out[3])

    def _status(self, check):
        return self._get(self.lib.tgnh_get_status_flags, C.c_uint32, stream=True, check=check)

    def status_flags(self):
        """The device's status word (bit 0 Drude beyond 2x the hard wall, bit 1 harness SHAKE not converged or the direct solver's result outside the tolerance, bit 2 mailbox
        exchange timed out), whether or not it spells a failure (the call's own status is ignored).  Synchronises the stream."""
        return self._status(check=False)

    def check(self):
        """The status word; raises TgnhError for the failures among its bits: a Drude beyond 2x the hard wall in dualNH
        mode (Ref :311-312), a mailbox exchange that timed out.  Once seen, a failure is sticky in the library: every
        later step or query raises too."""
        return self._status(check=True)

    def last_kinetic_energies(self): return self._vec(self.lib.tgnh_get_last_kinetic_energies, self.num_thermostats())

    def last_scale_factors(self): return self._vec(self.lib.tgnh_get_last_scale_factors, self.num_thermostats())

    def compute_kinetic_energies(self):
        _check(self.lib.tgnh_compute_kinetic_energies(self.h, self._stream()))
        return self.last_kinetic_energies()

    def half_kick(self): _check(self.lib.tgnh_half_kick(self.h, self._stream()))

    def kinetic_energy(self):
        return self._get(self.lib.tgnh_get_kinetic_energy, C.c_double, int(self.ke_sum_valid), stream=True)

    # ---- clock and timing ----
    def time(self): return self._get(self.lib.tgnh_get_time, (C.c_double, C.c_int64))

    def set_time(self, time, step_count):
        """Context::setTime / setStepCount of a restored checkpoint."""
        _check(self.lib.tgnh_set_time(self.h, float(time), int(step_count)))

    def timing(self, on): _check(self.lib.tgnh_timing_enable(self.h, int(on)))

    def timing_read(self, kid): return self._get(self.lib.tgnh_timing_read, (C.c_double, C.c_int64), kid)

    def algorithmic_bytes(self, kid): return self._get(self.lib.tgnh_algorithmic_bytes, C.c_double, kid)
