"""The direct constraint solver beside the harness' SHAKE, mixed precision, timed with HIP events on the step's stream, on rigid SWM4
water at 2 M slots (400 000 clusters of 3 constraints) and on config 3's constrained ionic liquid (99 990 slots, 22 220 clusters of 1
and 2 constraints), each at constraint tolerances 1e-5 and 1e-10:
 * each stage inside real constrained steps -- begin_kick, [positions stage], begin_move, virtual sites, force, end_kick, [velocity
   stage], end_thermo -- so that both solvers work on what a step hands them (the harness' sweep count depends on it), one pair of
   events around the stage's call; one context per solver, from the same start;
 * the whole constrained step (HipContext.step) with direct_constraints on and off.
With read_probe's output as second argument (tools/micro/read_probe.hip, run on the same box) the new stages are also put against that
read-only ceiling for their bytes.  Prints one JSON line (and writes it to the file given as first argument): the figures for
profiles/constraints.md."""
import json, os, re, sys
import numpy as np
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, root)
import torch
from openmm_drudenose_amd import synth, DrudeTGNHIntegrator, HipContext
from openmm_drudenose_amd.build import source_sha
from openmm_drudenose_amd.drudetgnhplugin import _check

SYSTEMS = {"rigid water, 2 M slots": lambda: synth.water_box(400_000, rigid=True),
           "constrained ionic liquid, 99 990 slots": lambda: synth.ionic_liquid(2222, constrained=True)}
TOLS = (1e-5, 1e-10)
WARM, STEPS, REPEATS = 10, 30, 5


def context(s, g, ng, direct):
    it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)
    it.setMaxDrudeDistance(0.02)
    for _ in range(ng):
        it.addTempGroup()
    it._particleTempGroup = np.ascontiguousarray(g, np.int32)
    return HipContext(s, it, mode="TGNH", precision="mixed", direct_constraints=direct)


def stats(us):
    us = np.array(us)
    return {"calls": len(us), "min": float(us.min()), "median": float(np.median(us)), "max": float(us.max())}


def stage_times(ctx, direct, tol, steps):
    """-> (positions stage, velocity stage): us per call over `steps` real steps, the stage's call between two events"""
    lib, h = ctx.lib, ctx.h
    pos_stage = lib.tgnh_apply_constraints if direct else lib.tgnh_harness_shake_positions
    vel_stage = lib.tgnh_apply_velocity_constraints if direct else lib.tgnh_harness_shake_velocities
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(steps)]
    for e in ev:
        st = ctx._stream()
        _check(lib.tgnh_step_begin_kick(h, st))
        e[0].record(); _check(pos_stage(h, tol, st)); e[1].record()
        _check(lib.tgnh_step_begin_move(h, st))
        _check(lib.tgnh_harness_virtual_sites(h, st))
        ctx.compute_forces()
        _check(lib.tgnh_step_end_kick(h, st))
        e[2].record(); _check(vel_stage(h, tol, st)); e[3].record()
        _check(lib.tgnh_step_end_thermo(h, st))
    torch.cuda.synchronize()
    return [e[0].elapsed_time(e[1]) * 1e3 for e in ev], [e[2].elapsed_time(e[3]) * 1e3 for e in ev]


def step_time(ctx, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); ctx.step(steps); b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps


out = {"source_sha": source_sha(), "precision": "mixed", "device": torch.cuda.get_device_name(0), "steps_per_figure": STEPS, "repeats": REPEATS, "cases": []}
rates = []
if len(sys.argv) > 2:
    rates = [float(m.group(1)) for m in re.finditer(r"^flat .*?([\d.]+) TB/s", open(sys.argv[2]).read(), re.M)]
    if rates:
        out["read_probe_flat_TBps_best"] = max(rates)
for name, make in SYSTEMS.items():
    s, g, ng = make()
    atoms_in = int((s.cluster_atoms >= 0).sum())
    k = len(s.cluster_atoms)
    # the byte model, mixed precision.  New stages: a table row of 76 B per cluster (atoms 16, inverse masses 32, three squared distances
    # 24, pair word 4); per atom of a cluster posq 16 + posq_correction 16 read, posDelta (or velm) 32 read and 32 written.  The harness:
    # atoms 16 + distances 48 per cluster, and velm's 32 B per atom on top in the positions stage (read for the mass).
    model = {"direct": 76 * k + 96 * atoms_in, "harness_positions": 64 * k + 128 * atoms_in, "harness_velocities": 64 * k + 96 * atoms_in}
    ctxs = {direct: context(s, g, ng, direct) for direct in (False, True)}
    for tol in TOLS:
        case = {"system": name, "slots": s.num_particles, "clusters": k, "atoms_in_clusters": atoms_in, "tolerance": tol, "model_bytes": model}
        for direct, ctx in ctxs.items():
            ctx.integrator.setConstraintTolerance(tol)
            ctx.step(WARM)
            torch.cuda.synchronize()
            p, v = stage_times(ctx, direct, tol, STEPS)
            who = "direct" if direct else "harness"
            case[who + "_positions_us"], case[who + "_velocities_us"] = stats(p), stats(v)
            case[who + "_step_us"] = stats([step_time(ctx, STEPS) for _ in range(REPEATS)])
            case[who + "_status"] = ctx.check()
        for stage in ("positions", "velocities", "step"):
            case[stage + "_direct_over_harness"] = case["direct_" + stage + "_us"]["median"] / case["harness_" + stage + "_us"]["median"]
        if rates:
            ceiling = model["direct"] / max(rates) / 1e6
            case["direct_ceiling_us"] = ceiling
            case["direct_positions_fraction_of_ceiling"] = ceiling / case["direct_positions_us"]["median"]
            case["direct_velocities_fraction_of_ceiling"] = ceiling / case["direct_velocities_us"]["median"]
        out["cases"].append(case)
    for ctx in ctxs.values():
        ctx.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
print(json.dumps(out, default=float))
