"""The library's NonbondedForce (tgnh_compute_nonbonded_force) on the reference's water box (tests/water_test_system.py: 216 SWM4
waters, 1 080 slots, 4.2 nm) with every molecule displaced a little, replicated 4 x 4 x 6 times to 103 680 slots in a 16.8 x 16.8 x
25.2 nm box, cutoff 1.0 nm, in one precision (third argument, default mixed), timed with HIP events on the context's stream, one pair
of events around each call:
 * the call without and with want_energy (one memset and five launches: cell, scan, place, rank, pairs);
 * pairs inside the cutoff per second: the images are exact copies, so the box holds 96 x the pairs the 4.2 nm box holds, counted
   here on the host over all pairs of that one;
 * the share of TESTED pairs that were inside: a lane tests every member of the 27 cells around its own, counted here from the
   cells' populations;
 * beside it the harness' water_force_kernel on the 1 080-slot box (tgnh_harness_water_force), for scale: O(N^2), one work-group a
   molecule, SWM4 hard-wired.
The cell build's share of the time needs the launches apart: with the CSV of a `rocprofv3 --kernel-trace --stats` run of this very
tool as second argument (a run of its own), the four nb_cell / nb_scan / nb_place / nb_rank rows are put against all nb_* rows.
Prints one JSON line (and writes it to the file given as first argument): the figures for profiles/nonbonded_force.md."""
import csv, json, os, sys
import numpy as np
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import torch
from openmm_drudenose_amd import HipContext
from openmm_drudenose_amd.build import source_sha
from openmm_drudenose_amd.forces import NonbondedForce, NonbondedForces
from openmm_drudenose_amd.system import DrudeSystem
import water_test_system as wts

IMAGES = (4, 4, 6)
CUTOFF = 1.0
WARM, CALLS = 5, 40
Q = (1.71636, -1.71636, 0.55733, 0.55733, -1.11466)
SIGMA, EPS = 0.318395, 0.21094 * 4.184


def stats(us):
    us = np.array(us)
    return {"calls": len(us), "min": float(us.min()), "median": float(np.median(us)), "max": float(us.max())}


def event_times(call, calls):
    for _ in range(WARM):
        call()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record(); call(); b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def water_table(n_mol):
    f = NonbondedForce()
    for _ in range(n_mol):
        for m, q in enumerate(Q):
            f.addParticle(q, SIGMA if m == 0 else 0.0, EPS if m == 0 else 0.0)
    par = f.tables()[3]
    base = 5 * np.arange(n_mol)
    pairs = np.array([(i, j) for i in range(5) for j in range(i + 1, 5)])
    ep = (base[:, None, None] + pairs[None]).reshape(-1, 2).astype(np.int32)
    ex = np.tile([0.0, 1.0, 0.0], (len(ep), 1))
    return (NonbondedForce.CutoffPeriodic, CUTOFF, 78.3, par, ep, ex)


precision = sys.argv[3] if len(sys.argv) > 3 else "mixed"
out = {"source_sha": source_sha(), "precision": precision, "device": torch.cuda.get_device_name(0), "cutoff_nm": CUTOFF, "images": list(IMAGES)}
small = wts.build()
x1 = small.positions + np.repeat(np.random.default_rng(2).normal(0, 0.01, (216, 3)), 5, axis=0)
# pairs inside the cutoff in the 4.2 nm box: all pairs but the intramolecular ones, minimum image
d = x1[:, None, :] - x1[None, :, :]
d -= wts.BOX * np.rint(d / wts.BOX)
inside1 = ((d * d).sum(-1) < CUTOFF ** 2) & (np.arange(1080)[:, None] // 5 != np.arange(1080)[None, :] // 5)
shifts = np.array([(i, j, k) for i in range(IMAGES[0]) for j in range(IMAGES[1]) for k in range(IMAGES[2])], np.float64) * wts.BOX
copies = len(shifts)
x = (x1[None] + shifts[:, None]).reshape(-1, 3)
n = len(x)
box = tuple(wts.BOX * m for m in IMAGES)
base = 5 * np.arange(n // 5)
s = DrudeSystem(mass=np.tile([15.6, 0.4, 1.0, 1.0, 1.0], n // 5), pair_drude=base + 1, pair_parent=base, resid=np.repeat(np.arange(n // 5), 5),
                positions=x, velocities=np.zeros_like(x), name=f"{copies} images of the reference's water box")
ctx = HipContext(s, wts.integrator(), mode="TGNH", precision=precision)
ctx.setPeriodicBoxVectors((box[0], 0.0, 0.0), (0.0, box[1], 0.0), (0.0, 0.0, box[2]))
nb = NonbondedForces(ctx, water_table(n // 5))
out["slots"], out["terms"], out["box_nm"] = n, list(nb.num_terms), list(box)
nc = np.array([max(1, int(np.floor(e / (1.001 * CUTOFF)))) for e in box])
cell = np.minimum(((x / np.array(box) - np.floor(x / np.array(box))) * nc).astype(np.int64), nc - 1)
pop = np.zeros(tuple(nc), np.int64)
np.add.at(pop, tuple(cell.T), 1)
around = sum(np.roll(pop, (i, j, k), (0, 1, 2)) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1))
out["cells"], out["largest_cell"] = [int(v) for v in nc], int(pop.max())
out["pairs_inside"] = int(inside1.sum() // 2) * copies
out["ordered_pairs_tested"] = int((pop * around).sum())
out["inside_share_of_tested"] = 2 * out["pairs_inside"] / out["ordered_pairs_tested"]
out["call_us"] = stats(event_times(nb.compute, CALLS))
out["call_energy_us"] = stats(event_times(lambda: nb.compute(energy=True), CALLS))
out["energy_kJ_per_mol"] = list(nb.energy())
out["pairs_inside_per_second"] = out["pairs_inside"] / (out["call_us"]["median"] * 1e-6)
out["status"] = ctx.check()
ctx.close()
if len(sys.argv) > 2 and os.path.exists(sys.argv[2]):
    rows = {r["Name"]: float(r["TotalDurationNs"]) for r in csv.DictReader(open(sys.argv[2])) if "nb_" in r.get("Name", "")}
    build = sum(v for k, v in rows.items() if any(t in k for t in ("nb_cell", "nb_scan", "nb_place", "nb_rank")))
    out["cell_build_share"] = build / sum(rows.values()) if rows else "not measured: the kernel statistics hold no nb_ row"
else:
    out["cell_build_share"] = "not measured: no kernel statistics given"
# for scale: the harness' O(N^2) kernel on the 1 080-slot box
small.positions = x1
ctx = HipContext(small, wts.integrator(), mode="TGNH", precision=precision)
out["harness_water_force_1080_slots_us"] = stats(event_times(
    lambda: ctx.lib.tgnh_harness_water_force(ctx.h, wts.BOX, CUTOFF, ctx.force.data_ptr(), ctx._stream()), CALLS))
ctx.setPeriodicBoxVectors((wts.BOX, 0.0, 0.0), (0.0, wts.BOX, 0.0), (0.0, 0.0, wts.BOX))
nb = NonbondedForces(ctx, water_table(216))
out["call_1080_slots_us"] = stats(event_times(nb.compute, CALLS))
ctx.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
print(json.dumps(out, default=float))
