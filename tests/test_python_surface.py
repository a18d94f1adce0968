"""CPU tests of the Python surface over the C ABI (openmm_drudenose_amd.drudetgnhplugin): which library calls a context makes and
in which order, which calls invalidate the cached kinetic-energy sum, the public names and signatures, and the ctypes helpers.

The stepping tests drive a `HipContext.__new__(HipContext)` whose `lib` is a recording stand-in: every `tgnh_*` attribute appends its
own name to a list and returns 0.  No device and no built library are needed for them.  The expected sequences were read off the
single-module drudetgnhplugin.py that stood before the split by concern, and this file was run against that module too: all of it
passed there but the first case of test_capture_steps_refuses_before_any_capture, the one order the split changed on purpose.

tests/golden/python_surface.json holds what that single module exposed and what a host-only handle on synth.nacl() answered.  It
was written once, from the commit before the split, by
    python -c "import sys, json; sys.path.insert(0, 'tests'); import test_python_surface as t; json.dump(t.snapshot(), open('tests/golden/python_surface.json', 'w'), indent=1, sort_keys=True)"
and is not regenerated from the code under test."""
import hashlib
import inspect
import itertools
import json
import os
import types

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
import openmm_drudenose_amd.drudetgnhplugin as plugin
from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator, HipContext, HostTopology, TgnhError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "python_surface.json")
TOPOLOGIES = range(8)


# ---- the snapshot ----
def class_surface(cls):
    out = {}
    for name in dir(cls):
        if name.startswith("_"):
            continue
        v = inspect.getattr_static(cls, name)
        if isinstance(v, property):
            out[name] = "property"
        elif callable(v):
            out[name] = str(inspect.signature(v))
        else:
            out[name] = repr(v)
    return out


def surface():
    names = sorted(k for k, v in vars(plugin).items() if (not k.startswith("_") or k == "_check") and not isinstance(v, types.ModuleType))
    return {"names": names, "classes": {c.__name__: class_surface(c) for c in (HipContext, HostTopology, DrudeTGNHIntegrator)}}


def host_queries():
    s, _, _ = synth.nacl()
    t = HostTopology(s, integ())
    out = {"num_thermostats": t.num_thermostats(), "num_molecules": t.num_molecules(), "frame_count_all": t.frame_count(),
           "frame_count_skip_drude": t.frame_count(True),
           "topology": [[len(a), hashlib.sha1(a.tobytes()).hexdigest()] for a in map(t.topology, TOPOLOGIES)]}
    t.close()
    return out


def snapshot():
    return {"surface": surface(), "host_queries": host_queries()}


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


# ---- the stand-ins ----
def integ():
    return DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 3, True, True)


class RecordingLib:
    """every tgnh_* attribute appends its name to .calls and returns 0; .out[name] is what such a call leaves in its last argument"""

    def __init__(self, **out):
        self.calls, self.out = [], out

    def __getattr__(self, name):
        if not name.startswith("tgnh_"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append(name)
            if name in self.out:
                args[-1]._obj.value = self.out[name]
            return 0
        return fn


class Buffer:
    """stands for a device tensor: an address, and assignments that go nowhere"""

    def data_ptr(self):
        return 4096

    def __setitem__(self, key, value):
        pass


class FakeTorch:
    float32 = float64 = None

    def from_numpy(self, a):
        return self

    def to(self, *args):
        return self


def stand_in(constrained=False, mode="TGNH", force_fn=False, call_outs=False, harness_sites=None, **out):
    ctx = HipContext.__new__(HipContext)
    ctx.lib, ctx.h, ctx.n, ctx.integrator = RecordingLib(**out), 1, 4, integ()
    ctx._stream = lambda: None
    ctx.torch, ctx.dev, ctx.rdt, ctx.mdt, ctx.precision = FakeTorch(), None, None, None, _lib.PREC_DOUBLE
    ctx.force, ctx.x0, ctx.velm, ctx.posq, ctx.posq_corr = Buffer(), Buffer(), Buffer(), Buffer(), None
    ctx.mode = {"TGNH": _lib.MODE_TGNH, "dualNH": _lib.MODE_DUALNH}[mode]
    ctx.k_drude, ctx.k_tether, ctx.sites_packed, ctx.unpacked_sites = 1.0, 2.0, True, False
    ctx.constrained = constrained
    ctx._harness_sites = constrained if harness_sites is None else harness_sites
    ctx._has_clusters, ctx._only_library_sites, ctx.first_particle = constrained, False, 0
    ctx.force_fn = (lambda c: c.lib.calls.append("force_fn")) if force_fn else None
    ctx.drude_force = ctx.site_forces = call_outs
    ctx.state_hook = None
    ctx.ke_sum_valid = False
    return ctx


def release(ctx):
    ctx.h = None            # (nothing for __del__ to close)


# ---- (a) step() ----
def expected_step(constrained, mode, force_fn, call_outs, hook=False):
    """the calls of ONE step on the Python-loop paths, or None where one of the library's C loops runs the whole call"""
    if not force_fn and not call_outs:
        return None
    force = ["force_fn" if force_fn else "tgnh_harness_force"]
    if call_outs:
        force += ["tgnh_compute_drude_force", "tgnh_distribute_virtual_site_forces"]
    head = ["state_hook"] if hook else []
    if not constrained:
        return head + ["tgnh_step_begin"] + force + ["tgnh_step_end"]
    seq = head + ["tgnh_step_begin_kick", "tgnh_harness_shake_positions", "tgnh_apply_constraints", "tgnh_step_begin_move",
                  "tgnh_harness_virtual_sites", "tgnh_compute_virtual_sites"] + force + ["tgnh_step_end_kick"]
    if mode == "TGNH":
        seq += ["tgnh_harness_shake_velocities", "tgnh_apply_velocity_constraints"]
    return seq + ["tgnh_step_end_thermo"]


STEP_CASES = list(itertools.product((False, True), ("TGNH", "dualNH"), (False, True), (False, True)))


@pytest.mark.parametrize("constrained,mode,force_fn,call_outs", STEP_CASES)
def test_step_call_sequence(constrained, mode, force_fn, call_outs):
    ctx = stand_in(constrained, mode, force_fn, call_outs)
    ctx.step(2)
    one = expected_step(constrained, mode, force_fn, call_outs)
    want = ["tgnh_run_harness_constrained" if constrained else "tgnh_run_harness"] if one is None else one * 2
    assert ctx.lib.calls == want
    assert ctx.ke_sum_valid is True
    release(ctx)


@pytest.mark.parametrize("constrained,mode,force_fn,call_outs", STEP_CASES)
def test_step_state_hook_and_zero_steps(constrained, mode, force_fn, call_outs):
    """the hook: once per step and first in it, on the Python-loop paths only; step(0) on a C-loop path leaves ke_sum_valid alone"""
    ctx = stand_in(constrained, mode, force_fn, call_outs)
    ctx.state_hook = lambda c: c.lib.calls.append("state_hook")
    one = expected_step(constrained, mode, force_fn, call_outs, hook=True)
    for valid in (False, True):
        ctx.ke_sum_valid = valid
        ctx.step(0)
        assert ctx.ke_sum_valid is valid
    if one is None:
        assert ctx.lib.calls == ["tgnh_run_harness_constrained" if constrained else "tgnh_run_harness"] * 2
    else:
        assert ctx.lib.calls == []
    del ctx.lib.calls[:]
    ctx.step(2)
    assert ctx.lib.calls == (["tgnh_run_harness_constrained" if constrained else "tgnh_run_harness"] if one is None else one * 2)
    release(ctx)


def test_step_without_forces():
    ctx = stand_in()
    ctx.ke_sum_valid = False
    ctx.step_without_forces(0)
    assert ctx.ke_sum_valid is False
    ctx.step_without_forces(3)
    assert ctx.lib.calls == ["tgnh_run_steps"] * 2 and ctx.ke_sum_valid is True
    release(ctx)
    ctx = stand_in(constrained=True)
    with pytest.raises(TgnhError) as e:
        ctx.step_without_forces(1)
    assert e.value.status == _lib.ERR_STATE and str(e.value) == "step_without_forces: unconstrained systems only"
    assert ctx.lib.calls == []
    release(ctx)


def test_capture_steps_refuses_before_any_capture():
    """Every refusal of capture_steps comes before the device is touched (the stand-in's torch has no `cuda` at all).  The one
    order that changed with the split: forces=False on a constrained context used to be refused from inside an open capture."""
    for kwargs, forces, text in ((dict(constrained=True), False, "capture_steps(forces=False): unconstrained systems only"),
                                 (dict(force_fn=True), True, "capture_steps supports the harness force call-out only"),
                                 (dict(call_outs=True), True, "capture_steps supports the harness force call-out only")):
        ctx = stand_in(**kwargs)
        ctx.cm_motion_removal = ctx.velocity_rescaling = 0
        with pytest.raises(TgnhError) as e:
            ctx.capture_steps(2, forces=forces)
        assert e.value.status == _lib.ERR_STATE and str(e.value) == text and ctx.lib.calls == []
        release(ctx)
    ctx = stand_in(tgnh_get_time=3)                      # step count 3, removal every 2: refused, with the counts in the text
    ctx.cm_motion_removal, ctx.velocity_rescaling = 2, 0
    with pytest.raises(TgnhError) as e:
        ctx.capture_steps(4)
    assert e.value.status == _lib.ERR_STATE and "centre-of-mass removal every 2 steps" in str(e.value) and "(3)" in str(e.value)
    release(ctx)


# ---- (b) _minimize_batch() ----
@pytest.mark.parametrize("force_fn,call_outs,harness_sites,library_sites",
                         list(itertools.product((False, True), (False, True), (False, True), (0, 2))))
def test_minimize_batch_call_sequence(force_fn, call_outs, harness_sites, library_sites):
    ctx = stand_in(False, "TGNH", force_fn, call_outs, harness_sites=harness_sites, tgnh_get_num_virtual_sites=library_sites)
    ctx._minimize_batch(3)
    query = [] if harness_sites else ["tgnh_get_num_virtual_sites"]      # (`or`: asked only where the harness' table is empty)
    if not force_fn and not call_outs and not harness_sites and not library_sites:
        assert ctx.lib.calls == query + ["tgnh_run_harness_minimize"]
    else:
        place = (["tgnh_harness_virtual_sites"] if harness_sites else []) + ["tgnh_compute_virtual_sites"]
        force = ["force_fn" if force_fn else "tgnh_harness_force"]
        if call_outs:
            force += ["tgnh_compute_drude_force", "tgnh_distribute_virtual_site_forces"]
        one = (place if harness_sites or library_sites else []) + force + ["tgnh_minimize_iterate"]
        assert ctx.lib.calls == query + one * 3
    release(ctx)


# ---- (c) who writes velocities ----
WRITERS = {
    "removeCMMotion": (),
    "shift_velocities": ([0.0, 0.0, 0.1],),
    "scale_velocities": ([1.0, 1.0, 1.0],),
    "rescale_to_temperature": (),
    "set_velocity_rescaling": (5,),
    "setVelocitiesToTemperature": (300.0, 1),
    "apply_velocity_constraints": (),
    "setVelocities": (np.zeros((4, 3)),),
    "setPositions": (np.zeros((4, 3)),),
}
NOT_WRITERS = {
    "scale_positions": (1.01,),
    "wrap_molecules": (),
    "compute_virtual_sites": (),
    "compute_drude_force": (),
}


@pytest.mark.parametrize("name", sorted(WRITERS))
def test_velocity_writers_clear_the_cached_sum(name):
    ctx = stand_in()
    ctx.ke_sum_valid = True
    getattr(ctx, name)(*WRITERS[name])
    assert ctx.ke_sum_valid is False
    assert ctx.lib.calls, name
    release(ctx)


@pytest.mark.parametrize("name", sorted(NOT_WRITERS))
def test_other_calls_leave_the_cached_sum(name):
    ctx = stand_in()
    for valid in (True, False):
        ctx.ke_sum_valid = valid
        getattr(ctx, name)(*NOT_WRITERS[name])
        assert ctx.ke_sum_valid is valid
    assert len(ctx.lib.calls) == 2
    release(ctx)


def test_step_entry_points_and_the_cached_sum():
    ctx = stand_in()
    ctx.step_begin()
    assert ctx.ke_sum_valid is False                     # (as stand_in left it: step_begin says nothing about the sum)
    ctx.step_end()
    assert ctx.ke_sum_valid is True and ctx.lib.calls == ["tgnh_step_begin", "tgnh_step_end"]
    release(ctx)


# ---- (d) the public surface ----
def test_public_surface_is_the_snapshot():
    want, got = golden()["surface"], surface()
    assert got["names"] == want["names"]
    for cls in want["classes"]:
        assert got["classes"][cls] == want["classes"][cls], cls
    for name in want["names"]:
        assert hasattr(plugin, name)


def test_context_takes_attributes_of_the_callers():
    ctx = HipContext.__new__(HipContext)
    ctx.leg, ctx.exchange, ctx.rccl_site, ctx.graph_used, ctx.dominant_in_timed_region = "a", None, 0, False, "x"
    assert not hasattr(HipContext, "__slots__") and ctx.leg == "a"
    release(ctx)


# ---- (e) the helpers, on a host-only handle ----
@pytest.fixture(scope="module")
def host():
    s, _, _ = synth.nacl()
    t = HostTopology(s, integ())
    yield t
    t.close()


def test_host_queries_are_the_snapshot():
    assert host_queries() == golden()["host_queries"]


def test_host_handle_basics(host):
    assert host.n == 2500 and host.frame_count() == 2500 and host.frame_count(True) == 2500 - 512
    assert host.num_molecules() == 512 and host.molecules().shape == (2500,)
    assert host.num_virtual_sites == 0 and host.num_drude_force_terms == (0, 0)
    assert host.num_constraint_clusters() == 0 and host.step_path()[0] in ("tiled", "gather")
    dof, nkt = host.dof()
    assert dof.shape == nkt.shape == (host.num_thermostats(),)


def refused(call, text):
    with pytest.raises(TgnhError) as e:
        call()
    assert e.value.status == _lib.ERR_ARG and str(e.value) == text


def test_shape_refusals_keep_their_text(host):
    refused(lambda: host.set_molecules(np.zeros(2499, np.int32)), "set_molecules: one label per particle slot")
    refused(lambda: host.set_molecules(np.zeros((2500, 1), np.int32)), "set_molecules: one label per particle slot")
    refused(lambda: host.set_constraint_clusters(np.zeros((2, 4), np.int32), np.zeros((1, 6))),
            "set_constraint_clusters: one row of distances per cluster")
    refused(lambda: host.set_virtual_sites(np.zeros(2, np.int32), np.zeros((2, 4), np.int32), np.zeros((1, 12))),
            "set_virtual_sites: one kind, one row of atoms and one row of twelve parameters per site")
    refused(lambda: host.set_virtual_sites(np.zeros(1, np.int32), np.zeros((2, 4), np.int32), np.zeros((2, 12))),
            "set_virtual_sites: one kind, one row of atoms and one row of twelve parameters per site")
    refused(lambda: host.set_drude_force((np.zeros((2, 5), np.int32), np.zeros((1, 4)), np.zeros((0, 2), np.int32), np.zeros(0))),
            "set_drude_force: one row of four parameters per row of particles, one thole per screened pair")
    refused(lambda: host.set_drude_force((np.zeros((0, 5), np.int32), np.zeros((0, 4)), np.zeros((1, 2), np.int32), np.zeros(2))),
            "set_drude_force: one row of four parameters per row of particles, one thole per screened pair")
    refused(lambda: host.setPeriodicBoxVectors([3.0, 0, 0], [0, 3.0, 0], [0, 0, 3.0, 0]),
            "setPeriodicBoxVectors: three vectors of three components")
    with pytest.raises(ValueError):                      # (a size that is no whole number of rows: numpy's own refusal)
        host.set_constraint_clusters(np.zeros(5, np.int32), np.zeros(6))
    assert host.getPeriodicBoxVectors() is None and host.num_molecules() == 512
    host.setPeriodicBoxVectors([3.0, 0, 0], [0, 3.0, 0], [0, 0, 3.0])
    assert np.array_equal(host.getPeriodicBoxVectors(), 3.0 * np.eye(3))


def test_shape_refusals_of_a_context_keep_their_text():
    ctx = stand_in()
    ctx.ke_sum_valid = True
    refused(lambda: ctx.shift_velocities([0.0, 1.0]), "shift_velocities: dv must have three components")
    refused(lambda: ctx.scale_velocities(np.ones((2, 2))), "scale_velocities: factors must be a vector, one per thermostat")
    refused(lambda: ctx.scale_positions([1.0, 1.0]), "scale_positions: scale is a scalar or has three components")
    refused(lambda: plugin.minimize_desc(4, moving=[1, 0, 1]), "minimize: one mask entry per particle slot")
    refused(lambda: plugin.split_clusters(np.zeros((2, 4), np.int32), np.zeros((1, 6))), "split_clusters: one row of distances per cluster")
    assert ctx.lib.calls == [] and ctx.ke_sum_valid is True
    release(ctx)


def test_out_parameters_of_a_context():
    """the reads that take the stream, and the ones of another type than int"""
    ctx = stand_in(tgnh_get_pending_state=0x412, tgnh_get_kinetic_energy=1.5, tgnh_get_status_flags=5, tgnh_get_resident_kernel=2,
                   tgnh_harness_sites_kind=1, tgnh_algorithmic_bytes=64.0, tgnh_get_resident_work_groups=3)
    assert ctx.pending_state() == 0x412 and ctx.kinetic_energy() == 1.5 and ctx.status_flags() == 5 and ctx.check() == 5
    assert ctx.resident_kernel() == "wstep_kernel" and ctx.sites_kind() == "packed" and ctx.algorithmic_bytes(0) == 64.0
    assert ctx.resident_work_groups() == 3 and ctx.time() == (0.0, 0) and ctx.timing_read(0) == (0.0, 0)
    release(ctx)
