"""velinit_kernel at 5 M slots, mixed precision, HIP events on the launch stream; beside it the wall time of the host recipe
(synth._finish's draws + setVelocities).  Prints one JSON line (and writes it to the file given as argument): the figures for profiles/velinit.md."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch
from openmm_drudenose_amd import synth, DrudeTGNHIntegrator, HipContext
from openmm_drudenose_amd.build import source_sha

s, g, ng = synth.water_box(1_000_000)
it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)
ctx = HipContext(s, it, mode="TGNH", precision="mixed")
n = s.num_particles
for _ in range(3):                                           # warm-up (the first call also builds the partner table)
    ctx.setVelocitiesToTemperature(300.0, 1, 1.0)
torch.cuda.synchronize()
us = []
for k in range(20):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    ctx.setVelocitiesToTemperature(300.0, 100 + k, 1.0)
    b.record()
    b.synchronize()
    us.append(a.elapsed_time(b) * 1e3)
us = np.array(us)

def host_recipe(seed):
    """the draws of synth._finish, as the parent commit starts a run"""
    rng = np.random.default_rng(seed)
    mass, pd, pp = s.mass, s.pair_drude, s.pair_parent
    vel = np.zeros((n, 3))
    in_pair = np.zeros(n, bool); in_pair[pd] = True; in_pair[pp] = True
    sel = (mass > 0) & ~in_pair
    vel[sel] = rng.normal(0.0, 1.0, (int(sel.sum()), 3)) * np.sqrt(synth.KB * 300.0 / mass[sel])[:, None]
    m1, m2 = mass[pd], mass[pp]
    mt, mu = m1 + m2, m1 * m2 / (m1 + m2)
    vcm = rng.normal(0.0, 1.0, (m1.shape[0], 3)) * np.sqrt(synth.KB * 300.0 / mt)[:, None]
    vrel = rng.normal(0.0, 1.0, (m1.shape[0], 3)) * np.sqrt(synth.KB * 1.0 / mu)[:, None]
    vel[pd] = vcm - vrel * (m2 / mt)[:, None]
    vel[pp] = vcm + vrel * (m1 / mt)[:, None]
    return vel

draw_s, up_s = [], []
for k in range(3):
    t0 = time.perf_counter(); v = host_recipe(k); t1 = time.perf_counter()
    ctx.setVelocities(v); torch.cuda.synchronize(); t2 = time.perf_counter()
    draw_s.append(t1 - t0); up_s.append(t2 - t1)
out = {"source_sha": source_sha(), "slots": n, "precision": "mixed", "device": torch.cuda.get_device_name(0),
       "velinit_us": {"launches": len(us), "min": us.min(), "median": float(np.median(us)), "max": us.max(), "all": us.round(1).tolist()},
       "bytes_per_slot": 32 + 32 + 4, "TBps_at_median": n * 68 / np.median(us) / 1e6,
       "host_recipe_s": {"draws": draw_s, "setVelocities": up_s}}
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
print(json.dumps(out, default=float))
ctx.close()
