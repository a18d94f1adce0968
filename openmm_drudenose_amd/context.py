"""`HipContext`, the core: the constructor, the device arrays in OpenMM's layouts (posq real4, velm mixed4 with w = 1/m, force
int64 x 2^32 in three planes, posqCorrection in mixed precision) and their binding, and positions, velocities, forces, charges and
the harness' tether sites in and out.  torch is used for device memory, streams and torch.distributed only.  The rest of the class
comes from stepping.py, sharding.py and features.py, each a plain class over handle.Handle."""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import TgnhError, _check, f64, i32
from .features import Features
from .handle import _MODE, _PREC, split_clusters
from .sharding import Sharding
from .stepping import Stepping
from .synth import KB, K_DRUDE, K_TETHER


class HipContext(Stepping, Sharding, Features):
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
        self.k_drude = K_DRUDE if k_drude is None else k_drude
        self.k_tether = K_TETHER if k_tether is None else k_tether
        with torch.cuda.device(self.dev):
            self._open(system, integrator, mode, precision, device, flags, kB)
        n = self.n
        self._pushed_baths = (integrator.getTemperature(), integrator.getDrudeTemperature())   # what the handle was created at
        self._bath_epoch = 0
        self.first_particle = 0                              # a shard: the index of its first slot in the whole system (setVelocitiesToTemperature)
        self._hook = None
        self.cm_motion_removal = self.velocity_rescaling = 0
        if cm_motion_removal is not None:
            with torch.cuda.device(self.dev):
                self.set_cm_motion_removal(cm_motion_removal)
        if global_dof_sum is not None:                      # particle sharding: dof terms are additive over ranks
            self.set_global_dof_terms(global_dof_sum(self.local_dof_terms()))
        if allreduce is not None:
            self.set_allreduce(allreduce)

        self.rdt = rdt = torch.float32 if self.precision != _lib.PREC_DOUBLE else torch.float64
        self.mdt = mdt = torch.float32 if self.precision == _lib.PREC_SINGLE else torch.float64
        self.posq = torch.zeros((n, 4), dtype=rdt, device=self.dev)
        self.posq_corr = torch.zeros((n, 4), dtype=torch.float32, device=self.dev) if self.precision == _lib.PREC_MIXED else None
        self.velm = torch.zeros((n, 4), dtype=mdt, device=self.dev)
        self.force = torch.zeros(3 * self.padded, dtype=torch.int64, device=self.dev)
        self.pos_delta = torch.zeros((n, 4), dtype=mdt, device=self.dev)
        self.x0 = torch.zeros((n, 4), dtype=rdt, device=self.dev)        # harness tether sites, w = tether flag
        self.sites_packed = False
        self.unpacked_sites = False                                      # (tests: the harness force from x0 itself, the round-1 kernel)
        self.use_lattice_sites = bool(lattice_sites)                     # (tests: False keeps the packed sites where the lattice form would hold)
        inv = np.where(system.mass == 0.0, 0.0, 1.0 / np.where(system.mass == 0.0, 1.0, system.mass))
        self.velm[:, 3] = torch.from_numpy(inv).to(self.dev, mdt)
        self._bind(self.velm)
        integrator._context = self
        self.force_fn = self.state_hook = None
        self.ke_sum_valid = self.constrained = False
        self.site_forces = False           # True: every compute_forces() is followed by one distribute_site_forces()
        self.drude_force = False           # True: every compute_forces() adds the library's DrudeForce after force_fn (compute_drude_force)
        self._split_constraints(system, direct_constraints)
        table = self._assemble_sites(system, library_sites)
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

    def _split_constraints(self, system, direct_constraints):
        """the system's constraint clusters: to the harness' SHAKE, or (direct_constraints) those the direct solver takes to it"""
        self._has_clusters = system.cluster_atoms is not None and len(system.cluster_atoms) > 0
        self._harness_clusters = 0
        if not self._has_clusters:
            return
        harness = (system.cluster_atoms, system.cluster_dist)
        if direct_constraints:
            direct, harness = split_clusters(*harness)
            self.set_constraint_clusters(*direct)
        self._harness_clusters = len(harness[0])
        if self._harness_clusters:
            _check(self.lib.tgnh_harness_set_clusters(self.h, len(harness[0]), i32(harness[0])[1], f64(harness[1])[1]))
        self.constrained = True

    def _assemble_sites(self, system, library_sites):
        """the system's three-particle-average sites: to the harness' table, or (library_sites) appended to what goes to the
        library's -> that table (kinds, atoms, params), the system's own site table first"""
        self._harness_sites = False        # the harness' site table holds sites (the system's three-particle averages, unless library_sites)
        table = [np.zeros(0, np.int32), np.zeros((0, 4), np.int32), np.zeros((0, _lib.SITE_PARAMS))]
        if system.site_table_kinds is not None and len(system.site_table_kinds):
            table = [system.site_table_kinds, system.site_table_atoms, system.site_table_params]
        if system.site_atoms is not None and len(system.site_atoms):
            if library_sites:
                params = np.zeros((len(system.site_atoms), _lib.SITE_PARAMS))
                params[:, :3] = system.site_weights
                table = [np.concatenate([table[0], np.full(len(system.site_atoms), _lib.SITE_THREE_AVERAGE, np.int32)]),
                         np.concatenate([table[1], system.site_atoms]), np.concatenate([table[2], params])]
            else:
                _check(self.lib.tgnh_harness_set_virtual_sites(self.h, len(system.site_atoms), i32(system.site_atoms)[1],
                                                               f64(system.site_weights)[1]))
                self._harness_sites = True
            self.constrained = True        # the split path is the one with the virtual-site call-out
        self._only_library_sites = not self._has_clusters and not self._harness_sites     # what makes the context `constrained` is at most sites of the library's table
        return table

    # ---- plumbing ----
    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)

    def _bind(self, velm):
        """tgnh_bind_buffers: the context's arrays, with `velm` as the velocities"""
        _check(self.lib.tgnh_bind_buffers(self.h, self.posq.data_ptr(), self.posq_corr.data_ptr() if self.posq_corr is not None else None,
                                          velm.data_ptr(), self.force.data_ptr(), self.pos_delta.data_ptr()))

    def close(self):
        if getattr(self, "h", None):
            self.torch.cuda.synchronize(self.dev)
        super().close()

    def _state_changed(self):                                # DrudeTGNHIntegrator.cpp:166-170
        self._wrote_velocities()
        _check(self.lib.tgnh_state_changed(self.h))

    # ---- state (Context::setPositions / setVelocities / getState) ----
    def setPositions(self, pos):
        torch = self.torch
        self._state_changed()
        p = torch.from_numpy(np.ascontiguousarray(pos, np.float64)).to(self.dev)
        if self.precision == _lib.PREC_DOUBLE:
            self.posq[:, :3] = p
        else:
            hi = p.to(torch.float32)
            self.posq[:, :3] = hi
            if self.posq_corr is not None:
                self.posq_corr[:, :3] = (p - hi.to(torch.float64)).to(torch.float32)

    def getPositions(self):
        p = self.posq[:, :3].to(self.torch.float64)
        if self.posq_corr is not None:
            p = p + self.posq_corr[:, :3].to(self.torch.float64)
        return p.cpu().numpy()

    def setCharges(self, q):
        """posq.w of every slot (OpenMM keeps the charge there; setPositions leaves it alone).  No step kernel reads it."""
        self.posq[:, 3] = self.torch.from_numpy(np.ascontiguousarray(q, np.float64)).to(self.dev, self.rdt)

    def setVelocities(self, vel):
        self._state_changed()                                # (first: refused between the steps of a deferred sequence, and then nothing is written)
        self.velm[:, :3] = self.torch.from_numpy(np.ascontiguousarray(vel, np.float64)).to(self.dev, self.mdt)

    def getVelocities(self):
        self.flush()
        return self.velm[:, :3].to(self.torch.float64).cpu().numpy()

    def rebind_velocities(self, velm):
        """tgnh_bind_buffers with another velm array (same shape, type and device) and every other array as bound; the context
        steps on it from here on.  Refused (TGNH_ERR_STATE) while a deferred half kick is pending: flush first, or call it between
        step_begin and step_end.  The array that goes holds the current velocities when the call returns; what the new one holds
        is the caller's business (its w must be 1/m)."""
        if velm.shape != self.velm.shape or velm.dtype != self.velm.dtype or velm.device != self.velm.device or not velm.is_contiguous():
            raise TgnhError(_lib.ERR_ARG, "rebind_velocities: a contiguous array of velm's shape, type and device")
        self._bind(velm)
        old, self.velm = self.velm, velm
        return old

    def getForces(self):
        f = self.force.view(3, self.padded)[:, :self.n].to(self.torch.float64) / 4294967296.0
        return f.t().contiguous().cpu().numpy()

    def setForces(self, f):
        """Forces in kJ/mol/nm -> OpenMM fixed point (long long)(f * 2^32)."""
        t = self.torch.from_numpy(np.ascontiguousarray(f, np.float64)).to(self.dev)
        self.force.view(3, self.padded)[:, :self.n] = (t * 4294967296.0).to(self.torch.int64).t()

    # ---- the harness' tether sites ----
    def set_sites(self, x0):
        """Harness tether sites (stored in the position type, so float-rounded unless precision is double);
        every massive particle that is not a Drude particle is tethered."""
        self.x0[:, :3] = self.torch.from_numpy(np.ascontiguousarray(x0, np.float64)).to(self.dev, self.rdt)
        flag = (self.system.mass > 0)
        flag[self.system.pair_drude] = False
        self.x0[:, 3] = self.torch.from_numpy(flag.astype(np.float64)).to(self.dev, self.rdt)
        self.torch.cuda.synchronize(self.dev)
        lat, hint = getattr(self.system, "lattice", None), (0, 0, 0.0, None, 0)
        if lat is not None and self.use_lattice_sites:
            # (a hint only: the library checks every slot against it and packs the sites as before where it does not hold)
            hint = (int(lat[0]), int(lat[1]), float(lat[2]), f64(lat[3])[1], int(lat[4]))      # k, side, spacing, geom, first
        _check(self.lib.tgnh_harness_lattice_hint(self.h, *hint))
        _check(self.lib.tgnh_harness_pack_sites(self.h, self.x0.data_ptr()))
        self.sites_packed = True

    def sites_kind(self):
        """how the harness force finds its tether sites: 'x0' (explicit array), 'packed', 'lattice'"""
        return ("x0", "packed", "lattice")[self._get(self.lib.tgnh_harness_sites_kind)]

    def _x0_arg(self):
        """None (NULL: the library reads its packed copy) once set_sites has packed them, else the float4 / double4 array"""
        return None if self.sites_packed and not self.unpacked_sites else self.x0.data_ptr()

    def sites(self):
        """The tether sites exactly as the harness kernel sees them (for the oracle)."""
        return self.x0[:, :3].to(self.torch.float64).cpu().numpy()
