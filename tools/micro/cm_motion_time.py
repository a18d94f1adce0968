"""Centre-of-mass removal at 1 M waters (5 M slots), mixed precision, timed with HIP events on the step's stream: the three
launches of tgnh_remove_cm_motion (momentum pass, row sum, shift); the harness' one-work-group stand-in
(tgnh_harness_remove_cm_motion); and a torch restatement on the device (m = 1 / w, sums of m and m v, v -= P / M on the massive
rows).  With read_probe's output as second argument (tools/micro/read_probe.hip, run on the same box) the launches are also put
against that read-only ceiling for their bytes.  Prints one JSON line (and writes it to the file given as first argument): the
figures for profiles/cm_motion.md."""
import json, os, re, sys
import numpy as np
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, root)
import torch
from openmm_drudenose_amd import synth, DrudeTGNHIntegrator, HipContext
from openmm_drudenose_amd.build import source_sha

s, g, ng = synth.water_box(1_000_000)
it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)
ctx = HipContext(s, it, mode="TGNH", precision="mixed")
ctx.setVelocitiesToTemperature(300.0, 1, 1.0)
n = s.num_particles
drift = torch.tensor([0.3, -0.2, 0.1], dtype=ctx.mdt, device=ctx.dev)
massive = ctx.velm[:, 3] != 0


def drifted():
    """every timed call starts from velocities with a centre-of-mass motion to remove"""
    ctx.velm[massive, :3] += drift


def library():
    ctx.removeCMMotion()


def harness():
    assert ctx.lib.tgnh_harness_remove_cm_motion(ctx.h, ctx._stream()) == 0


def torch_way():
    w = ctx.velm[:, 3]
    m = torch.where(w != 0, 1.0 / w, torch.zeros_like(w))
    vcm = (m[:, None] * ctx.velm[:, :3]).sum(0) / m.sum()
    ctx.velm[:, :3] -= torch.where(w != 0, 1.0, 0.0)[:, None] * vcm


def timed(fn, warm, calls):
    ms = []
    for k in range(warm + calls):
        drifted()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warm:
            ms.append(a.elapsed_time(b))
    us = np.array(ms) * 1e3
    return {"calls": len(us), "min": us.min(), "median": float(np.median(us)), "max": us.max(), "all": us.round(1).tolist()}


out = {"source_sha": source_sha(), "slots": n, "precision": "mixed", "device": torch.cuda.get_device_name(0),
       "library_us": timed(library, 3, 30), "harness_us": timed(harness, 1, 5), "torch_us": timed(torch_way, 3, 30)}
left = ctx.momentum()
out["velocity_left"] = left.velocity.tolist()
# the byte model: the pass reads velm (32 B per slot), the shift reads and writes it (64 B per slot)
out["model_bytes"] = 96 * n
out["TBps_model_at_median"] = out["model_bytes"] / out["library_us"]["median"] / 1e6
if len(sys.argv) > 2:
    rates = [float(m.group(1)) for m in re.finditer(r"^flat .*?([\d.]+) TB/s", open(sys.argv[2]).read(), re.M)]
    if rates:
        out["read_probe_flat_TBps_best"] = max(rates)
        out["ceiling_us_model_bytes"] = out["model_bytes"] / max(rates) / 1e6
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
print(json.dumps(out, default=float))
ctx.close()
