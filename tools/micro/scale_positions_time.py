"""The barostat's trial move at 1 M waters (5 M slots), mixed precision, timed with HIP events on the step's stream:
tgnh_scale_positions without and with its snapshot, and tgnh_restore_positions; beside them the host way they replace
(getPositions -> numpy -> setPositions, wall clock) and a torch restatement on the device (index_add_ centroid, gather, add, the
hi / lo split).  With read_probe's output as second argument (tools/micro/read_probe.hip, run on the same box) the launches are
also put against that read-only ceiling for their bytes.  Prints one JSON line (and writes it to the file given as first
argument): the figures for profiles/scale_positions.md."""
import json, os, re, sys, time
import numpy as np
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, root)
import torch
from openmm_drudenose_amd import synth, DrudeTGNHIntegrator, HipContext
from openmm_drudenose_amd.build import source_sha

s, g, ng = synth.water_box(1_000_000)
it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)
ctx = HipContext(s, it, mode="TGNH", precision="mixed")
n = s.num_particles
SCALE = (1.0013, 0.9991, 1.0007)
up, down = np.array(SCALE), 1.0 / np.array(SCALE)          # every other call undoes the last: the box does not wander
mol = torch.from_numpy(ctx.molecules().astype(np.int64)).to(ctx.dev)
count = torch.bincount(mol).to(torch.float64)
sm1 = torch.tensor(SCALE, dtype=torch.float64, device=ctx.dev) - 1.0
turn = [0]


def scale(save):
    def fn():
        ctx.scale_positions(up if turn[0] % 2 == 0 else down, save=save)
        turn[0] += 1
    return fn


def restore():
    ctx.restore_positions()


def torch_way():
    x = ctx.posq[:, :3].to(torch.float64) + ctx.posq_corr[:, :3].to(torch.float64)
    c = torch.zeros((count.shape[0], 3), dtype=torch.float64, device=ctx.dev).index_add_(0, mol, x) / count[:, None]
    x = x + (c * sm1)[mol]
    hi = x.to(torch.float32)
    ctx.posq[:, :3] = hi
    ctx.posq_corr[:, :3] = (x - hi.to(torch.float64)).to(torch.float32)


def host_way():
    x = ctx.getPositions()
    c = np.stack([np.bincount(mol_h, x[:, a]) for a in range(3)], 1) / count_h[:, None]
    ctx.setPositions(x + (c * (up - 1.0))[mol_h])
    torch.cuda.synchronize()


mol_h = ctx.molecules()
count_h = np.bincount(mol_h).astype(np.float64)


def timed(fn, warm, calls):
    ms = []
    for k in range(warm + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if k >= warm:
            ms.append(a.elapsed_time(b))
    us = np.array(ms) * 1e3
    return {"calls": len(us), "min": us.min(), "median": float(np.median(us)), "max": us.max(), "all": us.round(1).tolist()}


def wall(fn, warm, calls):
    us = []
    for k in range(warm + calls):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        if k >= warm:
            us.append((time.perf_counter() - t) * 1e6)
    us = np.array(us)
    return {"calls": len(us), "min": us.min(), "median": float(np.median(us)), "max": us.max(), "all": us.round(0).tolist()}


out = {"source_sha": source_sha(), "slots": n, "molecules": ctx.num_molecules(), "precision": "mixed", "device": torch.cuda.get_device_name(0)}
out["scale_us"] = timed(scale(False), 4, 30)
out["scale_save_us"] = timed(scale(True), 4, 30)
out["restore_us"] = timed(restore, 3, 30)
out["torch_us"] = timed(torch_way, 2, 10)
out["host_us"] = wall(host_way, 1, 3)
# the byte model, mixed precision: posq + posq_correction read (32 B per slot) and written (32 B); 32 B more with the snapshot; the
# restore reads and writes 32 B each
out["model_bytes"] = {"scale": 64 * n, "scale_save": 96 * n, "restore": 64 * n}
out["TBps_model_at_median"] = {k: out["model_bytes"][k] / out[k + "_us"]["median"] / 1e6 for k in out["model_bytes"]}
if len(sys.argv) > 2:
    rates = [float(m.group(1)) for m in re.finditer(r"^flat .*?([\d.]+) TB/s", open(sys.argv[2]).read(), re.M)]
    if rates:
        out["read_probe_flat_TBps_best"] = max(rates)
        out["ceiling_us_model_bytes"] = {k: v / max(rates) / 1e6 for k, v in out["model_bytes"].items()}
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
print(json.dumps(out, default=float))
ctx.close()
