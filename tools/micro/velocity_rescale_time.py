"""tgnh_rescale_to_temperature at 1 M waters (5 M slots), mixed precision, timed with HIP events on the step's stream, beside its
two constituents alone -- a kinetic-energy query (tgnh_compute_kinetic_energies: the KE pass and its row sum) and one rescale
launch (tgnh_scale_velocities: tile_kernel<SCALE> with factors from scratch, plus the one-work-group launch that carries them) --
and beside the host recipe it replaces: getVelocities -> the integrator's decomposition in numpy with the topology in hand ->
setVelocities.  Prints one JSON line (and writes it to the file given as first argument): the figures for
profiles/velocity_rescale.md."""
import json, os, sys, time
import numpy as np
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, root)
import torch
from openmm_drudenose_amd import synth, DrudeTGNHIntegrator, HipContext
from openmm_drudenose_amd.build import source_sha

T, TD = 350.0, 2.0
s, g, ng = synth.water_box(1_000_000)
it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)
ctx = HipContext(s, it, mode="TGNH", precision="mixed")
ctx.setVelocitiesToTemperature(300.0, 1, 1.0)
n = s.num_particles
start = ctx.velm.clone()
dof = ctx.dof()[0]
kB = ctx.dof()[1][0] / (dof[0] * it.getTemperature())
target = dof * kB * np.array([T, T, TD])
near_one = np.array([1.0 + 1e-9, 1.0 - 1e-9, 1.0 + 1e-9])
mass = np.asarray(s.mass, np.float64)
resid, pd, pp = np.asarray(s.resid), np.asarray(s.pair_drude), np.asarray(s.pair_parent)


def fresh():
    """every timed call starts from the drawn velocities"""
    ctx._state_changed()
    ctx.velm.copy_(start)


def rescale():
    ctx.rescale_to_temperature(T, TD)


def ke_query():
    assert ctx.lib.tgnh_compute_kinetic_energies(ctx.h, ctx._stream()) == 0


def scale_launch():
    ctx.scale_velocities(near_one)


def host_recipe():
    """one group, COM group on: v_com per molecule; a pair's centre of mass is an ordinary particle of mass m_d + m_p, its relative
    motion v_p - v_d has the reduced mass; three sums, three factors, the velocities put together again"""
    v = ctx.getVelocities()
    M = np.bincount(resid, mass)
    vcom = np.stack([np.bincount(resid, mass * v[:, k]) for k in range(3)], 1) / M[:, None]
    rel = v - vcom[resid]
    md, mp = mass[pd], mass[pp]
    mt = md + mp
    pcm = (md[:, None] * rel[pd] + mp[:, None] * rel[pp]) / mt[:, None]
    prel = rel[pp] - rel[pd]
    single = np.ones(n, bool)
    single[pd] = False
    single[pp] = False
    ke = np.array([(mass[single, None] * rel[single] ** 2).sum() + (mt[:, None] * pcm ** 2).sum(), (M[:, None] * vcom ** 2).sum(),
                   ((md * mp / mt)[:, None] * prel ** 2).sum()])
    f = np.sqrt(target / ke)
    out = f[0] * rel
    out[pd] = f[0] * pcm - f[2] * prel * (mp / mt)[:, None]
    out[pp] = f[0] * pcm + f[2] * prel * (md / mt)[:, None]
    out += f[1] * vcom[resid]
    out[mass == 0] = v[mass == 0]
    ctx.setVelocities(out)
    return f


def timed(fn, warm, calls):
    ms = []
    for k in range(warm + calls):
        fresh()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warm:
            ms.append(a.elapsed_time(b))
    us = np.array(ms) * 1e3
    return {"calls": len(us), "min": us.min(), "median": float(np.median(us)), "max": us.max(), "all": us.round(1).tolist()}


def wall(fn, calls):
    out = []
    for _ in range(calls):
        fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    us = np.array(out)
    return {"calls": len(us), "min": us.min(), "median": float(np.median(us)), "max": us.max(), "all": us.round(0).tolist()}


out = {"source_sha": source_sha(), "slots": n, "precision": "mixed", "device": torch.cuda.get_device_name(0),
       "rescale_to_temperature_us": timed(rescale, 3, 30), "ke_query_us": timed(ke_query, 3, 30),
       "scale_velocities_us": timed(scale_launch, 3, 30)}
fresh()
rescale()
out["factors_library"] = ctx.rescale_factors().tolist()
out["miss_after_library"] = (np.abs(ctx.compute_kinetic_energies() - target) / target).tolist()
out["host_recipe_wall_us"] = wall(host_recipe, 3)
fresh()
out["factors_host_recipe"] = host_recipe().tolist()
out["miss_after_host_recipe"] = (np.abs(ctx.compute_kinetic_energies() - target) / target).tolist()
# the byte model (tgnh_algorithmic_bytes: state arrays only): the KE pass reads velm, the rescale reads and writes it
out["model_bytes"] = 96 * n
out["TBps_model_at_median"] = out["model_bytes"] / out["rescale_to_temperature_us"]["median"] / 1e6
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
print(json.dumps(out, default=float))
ctx.close()
