"""Ewald summation on the library's NonbondedForce (tgnh_set_nonbonded_ewald), beside the reaction-field call on the same handle:
the reference's water box (tests/water_test_system.py: 216 SWM4 waters, 1 080 slots, 4.2 nm) with every molecule displaced a little,
as it is, replicated 1 x 3 x 3 times (9 720 slots) and 4 x 4 x 6 times (103 680 slots), cutoff 1.0 nm, in one precision (third
argument, default mixed).  At each size the parameters are NonbondedForce.ewald_parameters' for the default tolerance 5e-4, so M
grows with the box: the point of the largest size is to put on record where the explicit O(n M) sum stops being usable.  Timed
with HIP events on the context's stream, one pair of events around each call, after warm-up calls:
 * the reaction-field call (one memset and five launches);
 * the call with kmax (0, 0, 0): the erfc pairs and the exclusion correction, no reciprocal part;
 * the whole call; the reciprocal part's three launches are the difference to the line above.
The split of the reciprocal part by kernel needs the launches apart: with the CSV of a `rocprofv3 --kernel-trace --stats` run of this
very tool as second argument (a run of its own), the ew_* and nb_pair_ewald rows are listed by their share of the tool's whole run.
Prints one JSON line (and writes it to the file given as first argument): the figures for profiles/ewald.md."""
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

SIZES = ((1, 1, 1), (1, 3, 3), (4, 4, 6))
CUTOFF = 1.0
Q = (1.71636, -1.71636, 0.55733, 0.55733, -1.11466)
SIGMA, EPS = 0.318395, 0.21094 * 4.184


def stats(us):
    us = np.array(us)
    return {"calls": len(us), "min": float(us.min()), "median": float(np.median(us)), "max": float(us.max())}


def event_times(call, warm, calls):
    for _ in range(warm):
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
out = {"source_sha": source_sha(), "precision": precision, "device": torch.cuda.get_device_name(0), "cutoff_nm": CUTOFF, "tolerance": 5e-4, "sizes": []}
x1 = wts.build().positions + np.repeat(np.random.default_rng(2).normal(0, 0.01, (216, 3)), 5, axis=0)
rule = NonbondedForce()
rule.setCutoffDistance(CUTOFF)
for images in SIZES:
    shifts = np.array([(i, j, k) for i in range(images[0]) for j in range(images[1]) for k in range(images[2])], np.float64) * wts.BOX
    x = (x1[None] + shifts[:, None]).reshape(-1, 3)
    n = len(x)
    box = tuple(wts.BOX * m for m in images)
    base = 5 * np.arange(n // 5)
    s = DrudeSystem(mass=np.tile([15.6, 0.4, 1.0, 1.0, 1.0], n // 5), pair_drude=base + 1, pair_parent=base, resid=np.repeat(np.arange(n // 5), 5),
                    positions=x, velocities=np.zeros_like(x), name=f"{len(shifts)} images of the reference's water box")
    ctx = HipContext(s, wts.integrator(), mode="TGNH", precision=precision)
    ctx.setPeriodicBoxVectors((box[0], 0.0, 0.0), (0.0, box[1], 0.0), (0.0, 0.0, box[2]))
    nb = NonbondedForces(ctx, water_table(n // 5))
    alpha, kx, ky, kz = rule.ewald_parameters(box)
    warm, calls = (5, 40) if n < 50000 else (1, 5)               # (the largest size takes seconds a call)
    row = {"slots": n, "box_nm": list(box), "alpha": alpha, "kmax": [kx, ky, kz]}
    row["reaction_field_us"] = stats(event_times(nb.compute, warm, calls))
    nb.set_ewald(alpha, 0, 0, 0)
    row["direct_and_exclusions_us"] = stats(event_times(nb.compute, warm, calls))
    nb.set_ewald(alpha, kx, ky, kz)
    row["vectors"] = nb.ewald[2]
    row["ewald_us"] = stats(event_times(nb.compute, warm, calls))
    row["ewald_energy_us"] = stats(event_times(lambda: nb.compute(energy=True), warm, calls))
    row["reciprocal_us"] = row["ewald_us"]["median"] - row["direct_and_exclusions_us"]["median"]
    row["phase_factors_per_second"] = 2.0 * n * row["vectors"] / (row["reciprocal_us"] * 1e-6)      # the sum and the force launch: one each per (slot, vector)
    row["energy_kJ_per_mol"] = list(nb.energy() + nb.ewald_energy())
    row["status"] = ctx.check()
    out["sizes"].append(row)
    ctx.close()
if len(sys.argv) > 2 and os.path.exists(sys.argv[2]):
    rows = {r["Name"]: float(r["TotalDurationNs"]) for r in csv.DictReader(open(sys.argv[2])) if "ew_" in r.get("Name", "") or "nb_" in r.get("Name", "")}
    total = sum(rows.values())
    out["kernel_shares"] = {k: v / total for k, v in sorted(rows.items(), key=lambda kv: -kv[1])} if rows else "not measured: the kernel statistics hold no ew_ or nb_ row"
else:
    out["kernel_shares"] = "not measured: no kernel statistics given"
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
print(json.dumps(out, default=float))
