"""The periodic wrap and the frame at 1 M waters (5 M slots), mixed precision, timed with HIP events on the step's stream:
tgnh_wrap_molecules with nothing to move (every centre inside the cell: a read-only pass) and with every molecule moved (the
positions are shifted by one box vector before each timed call, outside the events), tgnh_write_frame plain and wrapped, with and
without the Drude particles, in both layouts, and the frame plus its copy to the host; beside them the host way they replace
(getPositions -> numpy: centroids by bincount, floor, subtract, float32; wall clock).  With read_probe's output as second argument
(tools/micro/read_probe.hip, run on the same box) the launches are also put against that read-only ceiling for their bytes.
Prints one JSON line (and writes it to the file given as first argument): the figures for profiles/wrap_frame.md."""
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
inside = s.positions - s.positions.min(0) + 0.5             # every centre well inside [0, L)
L = float(inside.max()) + 0.5
ctx.setPositions(inside)
ctx.setPeriodicBoxVectors((L, 0, 0), (0, L, 0), (0, 0, L))
kept = ctx.frame_count(True)
planes = torch.empty((3, n), dtype=torch.float32, device=ctx.dev)
rows = torch.empty((n, 3), dtype=torch.float32, device=ctx.dev)
planes_kept = torch.empty((3, kept), dtype=torch.float32, device=ctx.dev)
pinned = torch.empty((3, kept), dtype=torch.float32).pin_memory()
ctx.wrap_molecules()                                         # the device tables, outside the timed calls
ctx.frame(skip_drude=True, planes=True, out=planes_kept)


def push_out():
    ctx.posq[:, 0] += L                                      # one box vector: every molecule leaves the cell, and the wrap brings it back


def frame_to_host():
    ctx.frame(wrap=True, skip_drude=True, unit=10.0, planes=True, out=planes_kept)
    pinned.copy_(planes_kept, non_blocking=True)


mol_h = ctx.molecules()
count_h = np.bincount(mol_h).astype(np.float64)


def host_way():
    x = ctx.getPositions()
    c = np.stack([np.bincount(mol_h, x[:, a]) for a in range(3)], 1) / count_h[:, None]
    return ((x - (np.floor(c / L) * L)[mol_h]) * 10.0).astype(np.float32)


def timed(fn, warm, calls, prep=None):
    ms = []
    for k in range(warm + calls):
        if prep is not None:
            prep()
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


out = {"source_sha": source_sha(), "slots": n, "kept": kept, "molecules": ctx.num_molecules(), "precision": "mixed", "box_nm": L,
       "device": torch.cuda.get_device_name(0)}
out["wrap_none_us"] = timed(ctx.wrap_molecules, 4, 30)
out["wrap_all_us"] = timed(ctx.wrap_molecules, 4, 30, prep=push_out)
out["frame_plain_rows_us"] = timed(lambda: ctx.frame(out=rows), 4, 30)
out["frame_plain_planes_us"] = timed(lambda: ctx.frame(unit=10.0, planes=True, out=planes), 4, 30)
out["frame_wrap_planes_us"] = timed(lambda: ctx.frame(wrap=True, unit=10.0, planes=True, out=planes), 4, 30)
out["frame_wrap_kept_us"] = timed(lambda: ctx.frame(wrap=True, skip_drude=True, unit=10.0, planes=True, out=planes_kept), 4, 30)
out["frame_plain_kept_us"] = timed(lambda: ctx.frame(skip_drude=True, unit=10.0, planes=True, out=planes_kept), 4, 30)
out["frame_to_host_us"] = timed(frame_to_host, 2, 10)
out["host_us"] = wall(host_way, 1, 3)
# the byte model, mixed precision: posq + posq_correction read (32 B per slot); the wrap writes 32 B per moved slot; a frame writes
# 12 B per kept slot (the plain frame without Drude slots reads 4 B of out_index per slot more)
out["model_bytes"] = {"wrap_none": 32 * n, "wrap_all": 64 * n, "frame_plain_rows": 44 * n, "frame_plain_planes": 44 * n,
                      "frame_wrap_planes": 44 * n, "frame_wrap_kept": 32 * n + 12 * kept, "frame_plain_kept": 36 * n + 12 * kept}
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
