"""One FIRE iteration at 1 M waters (5 M slots), mixed precision.  Every leg runs in a fresh child process (the parent never opens
the GPU) and is timed with HIP events on the stream between two synchronisations, the host way by wall clock:
  iterate    tgnh_minimize_iterate, a minimisation under way: sums pass, row sum + decision, update pass
  sums       the same call on a minimisation that has converged: the update launch returns at once, so this is the sums pass, the
             row sum and an empty launch -- the update pass is `iterate` minus this
  force      the harness force call-out, apart
  step       one integrator step with its force call-out (tgnh_run_harness), for scale
  host       what the iteration replaces: getPositions + getForces, FIRE in numpy, setPositions
With read_probe's output as second argument (tools/micro/read_probe.hip, run on the same box in the same job) the passes are put
against that read-only ceiling for their model bytes.  Prints one JSON line (and writes it to the file given as first argument): the
figures for profiles/minimize.md."""
import json, os, re, subprocess, sys, time
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, root)
LEGS = ("iterate", "sums", "force", "step", "host")


def leg(name):
    import numpy as np
    import torch
    from openmm_drudenose_amd import synth, DrudeTGNHIntegrator, HipContext
    s, g, ng = synth.water_box(1_000_000)
    it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, 1, True, True)
    ctx = HipContext(s, it, mode="TGNH", precision="mixed")
    n = s.num_particles
    rng = np.random.default_rng(7)
    pos = s.positions + rng.normal(0.0, 0.02, s.positions.shape)
    pos[s.pair_drude] = pos[s.pair_parent] + rng.normal(0.0, 0.003, (s.num_pairs, 3))
    ctx.setPositions(pos)
    ctx.compute_forces()
    mask = s.mass != 0

    def timed(fn, warm, calls):
        ms = []
        for k in range(warm + calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if k >= warm:
                ms.append(a.elapsed_time(b))
        us = np.array(ms) * 1e3
        return {"calls": len(us), "min": us.min(), "median": float(np.median(us)), "max": us.max(), "all": us.round(1).tolist()}

    def host_way():
        # one iteration the host way: everything over PCIe and back (first-iteration mix: a = 1, b = 0)
        x, f = ctx.getPositions(), ctx.getForces()
        v = 1e-4 * f[mask]
        d = 1e-4 * v
        r = np.sqrt((d * d).sum(1))
        over = r > 0.01
        d[over] *= (0.01 / r[over])[:, None]
        x[mask] += d
        ctx.setPositions(x)
        torch.cuda.synchronize()

    if name == "iterate":
        ctx.minimize_begin(0.0)                      # tolerance 0: never converges
        out = timed(ctx.minimize_iterate, 4, 30)
        out["state"] = repr(ctx.minimize_state())
    elif name == "sums":
        ctx.minimize_begin(1e30)                     # the first decision converges; every later update launch returns at once
        ctx.minimize_iterate()
        assert ctx.minimize_state().converged == 1
        out = timed(ctx.minimize_iterate, 4, 30)
    elif name == "force":
        out = timed(ctx.compute_forces, 4, 30)
    elif name == "step":
        out = timed(lambda: ctx.step(1), 6, 30)
    elif name == "host":
        us = []
        for k in range(4):
            torch.cuda.synchronize()
            t = time.perf_counter()
            host_way()
            if k >= 1:
                us.append((time.perf_counter() - t) * 1e6)
        us = np.array(us)
        out = {"calls": len(us), "min": us.min(), "median": float(np.median(us)), "max": us.max(), "all": us.round(0).tolist()}
    out["slots"], out["moving"], out["device"] = n, int(mask.sum()), torch.cuda.get_device_name(0)
    print("LEG " + json.dumps(out, default=float))
    ctx.close()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--leg":
        leg(sys.argv[2])
        sys.exit(0)
    from openmm_drudenose_amd.build import source_sha
    out = {"source_sha": source_sha(), "precision": "mixed"}
    for name in LEGS:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name], capture_output=True, text=True, timeout=280)
        line = [x for x in r.stdout.splitlines() if x.startswith("LEG ")]
        if r.returncode != 0 or not line:          # a leg that failed ends the job: nothing more is started on the device
            print(json.dumps({"failed_leg": name, "returncode": r.returncode, "stderr": r.stderr[-2000:]}))
            sys.exit(1)
        out[name + "_us"] = json.loads(line[0][4:])
    n, moving = out["iterate_us"]["slots"], out["iterate_us"]["moving"]
    out["slots"], out["moving"] = n, moving
    # the byte model, mixed precision, per MOVING slot (4 of a water's 5): the sums pass reads F 24 + v 24; the update reads F 24
    # and v 24, writes v 24, reads and writes x 32 each; per slot of either kind the mask byte, once per pass
    out["model_bytes"] = {"sums": 48 * moving + n, "update": 136 * moving + n}
    med = {k: out[k + "_us"]["median"] for k in LEGS}
    out["update_us_by_difference"] = med["iterate"] - med["sums"]
    out["TBps_model"] = {"sums": out["model_bytes"]["sums"] / med["sums"] / 1e6,
                         "update": out["model_bytes"]["update"] / max(out["update_us_by_difference"], 1e-9) / 1e6}
    if len(sys.argv) > 2:
        rates = [float(m.group(1)) for m in re.finditer(r"^flat .*?([\d.]+) TB/s", open(sys.argv[2]).read(), re.M)]
        if rates:
            out["read_probe_flat_TBps_best"] = max(rates)
            out["ceiling_us_model_bytes"] = {k: v / max(rates) / 1e6 for k, v in out["model_bytes"].items()}
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1, default=float)
    print(json.dumps(out, default=float))
