"""tgnh_get_drude_statistics at 1 M pairs (5 M slots), mixed precision: the call between two synchronisations (a host clock: the
call ends in its own stream synchronise), and beside it what a user does without it -- getPositions() to the host plus the numpy
restatement of the header (tests/test_drude_stats.py's `stats`).  With read_probe's output as second argument
(tools/micro/read_probe.hip, run on the same box) the call is also put against that read-only ceiling for the pass's bytes.
Prints one JSON line (and writes it to the file given as first argument): the figures for profiles/drude_stats.md."""
import json, os, re, sys, time
import numpy as np
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import torch
from openmm_drudenose_amd import synth, DrudeTGNHIntegrator, HipContext
from openmm_drudenose_amd.build import source_sha
from test_drude_stats import stats, configure, THRESHOLD, HIST_MAX

s, g, ng = synth.water_box(1_000_000)
pos, q = configure(s)
it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)
ctx = HipContext(s, it, mode="TGNH", precision="mixed")
ctx.setPositions(pos)
ctx.setCharges(q)
n, P = s.num_particles, s.num_pairs
for _ in range(3):                                           # warm-up (the first call also builds the partner table and allocates the rows)
    got = ctx.drude_statistics(THRESHOLD, HIST_MAX)
torch.cuda.synchronize()
us = []
for k in range(30):
    t0 = time.perf_counter()
    got = ctx.drude_statistics(THRESHOLD, HIST_MAX)          # (synchronises the stream itself)
    us.append((time.perf_counter() - t0) * 1e6)
us = np.array(us)
host = []
for k in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter(); p = ctx.getPositions(); t1 = time.perf_counter()
    ref = stats(s, p, q, "double", THRESHOLD, HIST_MAX); t2 = time.perf_counter()      # (the positions come back as doubles: nothing left to split)
    host.append((t1 - t0, t2 - t1))
same = (got.pairs, got.over, got.worst_particle) == (ref.pairs, ref.over, ref.worst_particle) and np.array_equal(got.hist, ref.hist)
# the issue's model: 4 B of index per slot + 32 B per pair for posq of both members, as much again for the correction
model_bytes = 4 * n + 64 * P
# what the memory system moves where pairs are dense: every line of posq and of the correction holds a pair member
line_bytes = (4 + 16 + 16) * n
out = {"source_sha": source_sha(), "slots": n, "pairs": P, "precision": "mixed", "device": torch.cuda.get_device_name(0),
       "call_us": {"calls": len(us), "min": us.min(), "median": float(np.median(us)), "max": us.max(), "all": us.round(1).tolist()},
       "model_bytes": model_bytes, "whole_array_bytes": line_bytes,
       "TBps_model_at_median": model_bytes / np.median(us) / 1e6, "TBps_whole_arrays_at_median": line_bytes / np.median(us) / 1e6,
       "host_way_s": {"getPositions": [h[0] for h in host], "numpy": [h[1] for h in host]},
       "integers_agree_with_host_way": bool(same)}
if len(sys.argv) > 2:
    rates = [float(m.group(1)) for m in re.finditer(r"^flat .*?([\d.]+) TB/s", open(sys.argv[2]).read(), re.M)]
    if rates:
        out["read_probe_flat_TBps_best"] = max(rates)
        out["ceiling_us_model_bytes"] = model_bytes / max(rates) / 1e6
        out["ceiling_us_whole_arrays"] = line_bytes / max(rates) / 1e6
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
print(json.dumps(out, default=float))
ctx.close()
