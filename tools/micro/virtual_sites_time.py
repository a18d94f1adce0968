"""The library's virtual-site stage on rigid SWM4 water at 2 M slots (400 000 three-particle-average M sites), mixed precision, timed
with HIP events on the context's stream:
 * placement: tgnh_compute_virtual_sites beside the harness' site_kernel (tgnh_harness_virtual_sites), one context each, the same
   positions, one pair of events around each call;
 * distribution: tgnh_distribute_virtual_site_forces on a force buffer with forces on every slot, beside the host way -- getForces
   (device to host), the three shares added in numpy, setForces (host to device) -- timed on the wall clock between two
   synchronisations.
With read_probe's output as second argument (tools/micro/read_probe.hip, run on the same box) the two launches are also put against
that read-only ceiling for their bytes.  Prints one JSON line (and writes it to the file given as first argument): the figures for
profiles/virtual_sites.md."""
import json, os, re, sys, time
import numpy as np
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, root)
import torch
from openmm_drudenose_amd import synth, DrudeTGNHIntegrator, HipContext
from openmm_drudenose_amd.build import source_sha
from openmm_drudenose_amd.drudetgnhplugin import _check

MOLECULES = 400_000
WARM, CALLS, HOST_CALLS = 5, 40, 3


def context(s, g, ng, library):
    it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)
    it.setMaxDrudeDistance(0.02)
    for _ in range(ng):
        it.addTempGroup()
    it._particleTempGroup = np.ascontiguousarray(g, np.int32)
    return HipContext(s, it, mode="TGNH", precision="mixed", library_sites=library)


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


out = {"source_sha": source_sha(), "precision": "mixed", "device": torch.cuda.get_device_name(0), "molecules": MOLECULES}
rates = []
if len(sys.argv) > 2:
    rates = [float(m.group(1)) for m in re.finditer(r"^flat .*?([\d.]+) TB/s", open(sys.argv[2]).read(), re.M)]
    if rates:
        out["read_probe_flat_TBps_best"] = max(rates)
s, g, ng = synth.water_box(MOLECULES, rigid=True)
n, sites = s.num_particles, len(s.site_atoms)
out["slots"], out["sites"] = n, sites
# the byte model, mixed precision.  Placement, per site: a table row of 44 B (atoms 16, kind 4, three weights 24), three parents'
# posq 16 + posq_correction 16 read, x, y, z of the site's own pair written (12 + 12; counted as the 32 B of the two slots): 172 B; the
# harness reads a row of 40 B and the site's posq (for its w) on top: 184 B.  Distribution, per receiving slot (three a molecule): slot
# 4, offsets 4, row 4, role 1, the site's table row atoms 16 + kind 4 + one weight 8, the site's force 24, the slot's own force read and
# written 48: 113 B.
model = {"placement": 172 * sites, "harness_placement": 184 * sites, "distribution": 113 * 3 * sites}
out["model_bytes"] = model
harness, library = context(s, g, ng, False), context(s, g, ng, True)
assert library.num_virtual_sites == sites and library.constraint_clusters[1] == sites
out["harness_placement_us"] = stats(event_times(lambda: _check(harness.lib.tgnh_harness_virtual_sites(harness.h, harness._stream())), CALLS))
out["placement_us"] = stats(event_times(library.compute_virtual_sites, CALLS))
out["placement_over_harness"] = out["placement_us"]["median"] / out["harness_placement_us"]["median"]
out["largest_difference_between_the_two_placements_nm"] = float(np.abs(harness.getPositions() - library.getPositions()).max())   # (the harness contracts its sums)
# forces on every slot, the sites included
f = torch.randn((3, library.padded), dtype=torch.float64, device=library.dev) * 1e3
library.force[:] = (f * 4294967296.0).to(torch.int64).reshape(-1)
start = library.force.clone()
out["distribution_us"] = stats(event_times(library.distribute_site_forces, CALLS))


def host_way():
    fh = library.getForces()
    sa, w = s.site_atoms, s.site_weights
    for m in range(3):
        np.add.at(fh, sa[:, 1 + m], w[:, [m]] * fh[sa[:, 0]])
    library.setForces(fh)


host = []
for _ in range(HOST_CALLS):
    library.force.copy_(start)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_way()
    torch.cuda.synchronize()
    host.append((time.perf_counter() - t0) * 1e6)
out["host_distribution_us"] = stats(host)
out["host_over_device"] = out["host_distribution_us"]["median"] / out["distribution_us"]["median"]
if rates:
    for key in ("placement", "distribution"):
        ceiling = model[key] / max(rates) / 1e6
        out[key + "_ceiling_us"] = ceiling
        out[key + "_fraction_of_ceiling"] = ceiling / out[key + "_us"]["median"]
out["status"] = [harness.check(), library.check()]
harness.close(); library.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
print(json.dumps(out, default=float))
