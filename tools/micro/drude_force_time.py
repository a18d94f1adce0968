"""The library's own DrudeForce (tgnh_compute_drude_force) on the bench shape -- SWM4 water, 1 M molecules = 1 M Drude pairs, 5 M
slots, mixed precision --, timed with HIP events on the context's stream, one pair of events around each call:
 * the bench shape's table: one isotropic row per pair, without and with want_energy;
 * a table with anisotropy and screened pairs on the same box: every row with both axes (p2 = H1; p3, p4 = H1, H2) and one screened
   pair per two neighbouring molecules, without and with want_energy;
 * beside them the harness' force_kernel (tgnh_harness_force: Drude spring + tether) on the same context.
With read_probe's output as second argument (tools/micro/read_probe.hip, run on the same box) the launches are also put against that
read-only ceiling for their bytes.  Prints one JSON line (and writes it to the file given as first argument): the figures for
profiles/drude_force.md.  A term is recomputed by every slot that receives from it; what a term-major two-launch form would have to
beat is the distance of these figures from the ceiling."""
import json, os, re, sys
import numpy as np
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, root)
import torch
from openmm_drudenose_amd import synth, DrudeTGNHIntegrator, HipContext
from openmm_drudenose_amd.build import source_sha
from openmm_drudenose_amd.forces import DrudeForce

MOLECULES = 1_000_000
WARM, CALLS = 5, 40
Q_D, ALPHA = -1.71636, 0.00097825                    # SWM4-NDP


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


def tables(s, anisotropic):
    """one row per pair of the water box (slots O, D, H1, H2, M per molecule) -> the four arrays of tgnh_set_drude_force"""
    d, o = np.asarray(s.pair_drude), np.asarray(s.pair_parent)
    n = len(d)
    none = np.full(n, -1)
    particles = np.stack([d, o, o + 2, o + 2, o + 3] if anisotropic else [d, o, none, none, none], 1).astype(np.int32)
    params = np.tile([Q_D, ALPHA, 1.05, 0.95], (n, 1))
    rows = np.arange(n - n % 2, dtype=np.int32).reshape(-1, 2) if anisotropic else np.zeros((0, 2), np.int32)
    return particles, params, rows, np.full(len(rows), 2.6)


out = {"source_sha": source_sha(), "precision": "mixed", "device": torch.cuda.get_device_name(0), "molecules": MOLECULES}
rates = []
if len(sys.argv) > 2:
    rates = [float(m.group(1)) for m in re.finditer(r"^flat .*?([\d.]+) TB/s", open(sys.argv[2]).read(), re.M)]
    if rates:
        out["read_probe_flat_TBps_best"] = max(rates)
s, g, ng = synth.water_box(MOLECULES)
it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)
it.setMaxDrudeDistance(0.02)
for _ in range(ng):
    it.addTempGroup()
it._particleTempGroup = np.ascontiguousarray(g, np.int32)
ctx = HipContext(s, it, mode="TGNH", precision="mixed")
pairs = s.num_pairs
out["slots"], out["pairs"] = s.num_particles, pairs
# the byte model, mixed precision: per receiving slot its list (slot 4, offsets 4) and its own force read and written (48), per entry
# (term 4, role 1) the term's row (atoms 16, p4 4, three constants 24) or pair (rows 8, constants 16, two rows' atoms 32), and posq 16 +
# posq_correction 16 of every position the role reads -- counted once per entry, although neighbouring lanes share most of them in cache.
SLOT, ENTRY, ROW, PAIR, POS = 56, 5, 44, 56, 32
model = {"isotropic": 2 * pairs * (SLOT + ENTRY + ROW + 2 * POS),                   # D and O, one entry each, two positions
         # D, O, H1, H2 receive; five row entries a molecule (H1 is p2 and p3), four positions each at most; four site entries a
         # screened pair, three positions each
         "anisotropic_screened": 4 * pairs * SLOT + 5 * pairs * (ENTRY + ROW + 4 * POS) + 4 * (pairs // 2) * (ENTRY + PAIR + 3 * POS),
         "force_kernel": s.num_particles * (32 + 24)}                               # posq + posq_correction read, three force entries written
out["model_bytes"] = model
out["force_kernel_us"] = stats(event_times(ctx.compute_forces, CALLS))
for name, anisotropic in (("isotropic", False), ("anisotropic_screened", True)):
    ctx.set_drude_force(tables(s, anisotropic))
    out[name + "_terms"] = list(ctx.num_drude_force_terms)
    out[name + "_us"] = stats(event_times(ctx.compute_drude_force, CALLS))
    out[name + "_energy_us"] = stats(event_times(lambda: ctx.compute_drude_force(energy=True), CALLS))
    out[name + "_energy_kJ_per_mol"] = list(ctx.drude_energy())
    out[name + "_over_force_kernel"] = out[name + "_us"]["median"] / out["force_kernel_us"]["median"]
    if rates:
        ceiling = model[name] / max(rates) / 1e6
        out[name + "_ceiling_us"] = ceiling
        out[name + "_fraction_of_ceiling"] = ceiling / out[name + "_us"]["median"]
out["status"] = ctx.check()
ctx.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
print(json.dumps(out, default=float))
