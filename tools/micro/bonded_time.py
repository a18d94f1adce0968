"""The library's bonded forces (tgnh_compute_bonded_forces) on the chain system of tests/test_bonded_forces.py -- 58 branched
eight-atom chains with Drude particles, 20 waters, 24 ions: 722 slots -- replicated to about 1 M slots, in one precision (third
argument, default mixed), timed with HIP events on the context's stream, one pair of events around each call:
 * the bonds alone, without and with want_energy;
 * bonds, angles and torsions, without and with want_energy;
 * beside them tgnh_compute_drude_force (the isotropic rows and one screened pair a chain of the same system) on the same context.
With read_probe's output as second argument (tools/micro/read_probe.hip, run on the same box) the launches are also put against that
read-only ceiling for their bytes.  Prints one JSON line (and writes it to the file given as first argument): the figures for
profiles/bonded_forces.md.  A term is recomputed by every slot that receives from it -- two to four times --; what a term-major
two-launch form would have to beat is the distance of these figures from the ceiling."""
import json, os, re, sys
import numpy as np
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import torch
from openmm_drudenose_amd import DrudeTGNHIntegrator, HipContext
from openmm_drudenose_amd.build import source_sha
from openmm_drudenose_amd.forces import BondedForces
from openmm_drudenose_amd.system import DrudeSystem
from test_bonded_forces import bonded_system

SLOTS = 1_000_000
WARM, CALLS = 5, 40


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


def replicate(copies):
    """`copies` images of the tests' system side by side along x, 6 nm apart: slots, rows and pairs of image c behind those of c - 1
    -> (the system, its DrudeForce tables, the three bonded tables)"""
    s, (bonds, angles, torsions), _ = bonded_system()
    n = s.num_particles
    off = (np.arange(copies, dtype=np.int64) * n)
    tile = lambda a: np.tile(a, (copies,) + (1,) * (a.ndim - 1))                                   # noqa: E731
    shift = lambda p: (p[None] + off.reshape((-1,) + (1,) * p.ndim)).reshape((-1,) + p.shape[1:]).astype(np.int32)   # noqa: E731
    pos = (s.positions[None] + np.stack([6.0 * np.arange(copies), np.zeros(copies), np.zeros(copies)], 1)[:, None]).reshape(-1, 3)
    particles, params, screened, thole = s.drude_force.tables()
    moved = particles[None].astype(np.int64) + np.where(particles >= 0, 1, 0)[None] * off[:, None, None]
    rows = (screened[None].astype(np.int64) + (np.arange(copies) * len(particles))[:, None, None]).reshape(-1, 2).astype(np.int32)
    big = DrudeSystem(mass=tile(s.mass), pair_drude=shift(s.pair_drude), pair_parent=shift(s.pair_parent),
                      resid=(s.resid[None] + (np.arange(copies) * (s.resid.max() + 1))[:, None]).reshape(-1).astype(np.int32),
                      positions=pos, velocities=tile(s.velocities), name=f"{copies} images of {s.name}")
    drude = (moved.reshape(-1, 5).astype(np.int32), tile(params), rows, tile(thole))
    return big, drude, ((shift(bonds[0]), tile(bonds[1])), (shift(angles[0]), tile(angles[1])), (shift(torsions[0]), tile(torsions[1]), tile(torsions[2])))


precision = sys.argv[3] if len(sys.argv) > 3 else "mixed"
out = {"source_sha": source_sha(), "precision": precision, "device": torch.cuda.get_device_name(0)}
rates = []
if len(sys.argv) > 2:
    rates = [float(m.group(1)) for m in re.finditer(r"^flat .*?([\d.]+) TB/s", open(sys.argv[2]).read(), re.M)]
    if rates:
        out["read_probe_flat_TBps_best"] = max(rates)
s, drude_tables, tables = replicate(SLOTS // bonded_system()[0].num_particles)
it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.0005, 20, 1, True, True)
ctx = HipContext(s, it, mode="TGNH", precision=precision)
ctx.set_drude_force(drude_tables)
out["slots"], out["pairs"] = s.num_particles, s.num_pairs
nb, na, nt = (len(t[0]) for t in tables)
recv_all = len(np.unique(np.concatenate([t[0].ravel() for t in tables])))
recv_bonds = len(np.unique(tables[0][0]))
# the byte model: per receiving slot its list (slot 4, offsets 4) and its own force read and written (48); per entry (term 4, role 1)
# the term's row (a bond: atoms 8, constants 16; an angle: 16 + 16; a torsion: 16 + 4 + 24) and the positions it reads (posq, and
# posq_correction in mixed precision) -- counted once per entry, although neighbouring lanes share most of them in cache.
POS = {"single": 16, "mixed": 32, "double": 32}[precision]
SLOT, ENTRY = 56, 5
bond_bytes, angle_bytes, torsion_bytes = 2 * nb * (ENTRY + 24 + 2 * POS), 3 * na * (ENTRY + 32 + 3 * POS), 4 * nt * (ENTRY + 44 + 4 * POS)
model = {"bonds": recv_bonds * SLOT + bond_bytes, "all": recv_all * SLOT + bond_bytes + angle_bytes + torsion_bytes}
out["model_bytes"], out["receivers"] = model, {"bonds": recv_bonds, "all": recv_all}
out["drude_force_terms"] = list(ctx.num_drude_force_terms)
out["drude_force_us"] = stats(event_times(ctx.compute_drude_force, CALLS))
for name, kw in (("bonds", dict(bonds=tables[0])), ("all", dict(bonds=tables[0], angles=tables[1], torsions=tables[2]))):
    f = BondedForces(ctx, **kw)
    out[name + "_terms"] = list(f.num_terms)
    out[name + "_us"] = stats(event_times(f.compute, CALLS))
    out[name + "_energy_us"] = stats(event_times(lambda: f.compute(energy=True), CALLS))
    out[name + "_energy_kJ_per_mol"] = list(f.energy())
    out[name + "_over_drude_force"] = out[name + "_us"]["median"] / out["drude_force_us"]["median"]
    if rates:
        ceiling = model[name] / max(rates) / 1e6
        out[name + "_ceiling_us"] = ceiling
        out[name + "_fraction_of_ceiling"] = ceiling / out[name + "_us"]["median"]
out["status"] = ctx.check()
ctx.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
print(json.dumps(out, default=float))
