"""bench.py on one GPU: a plain run is the headline alone (set-up, warm-up, exactly --steps timed steps, one line), --full adds
what takes runs of its own, and --dump-outputs writes what the timed steps computed.  Both take the dump right after the timed
region, and the library is reproducible bit for bit on one device (include/drude_tgnh.h), so both write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
MOVED = {"kernels", "roofline", "integrator_only", "extra", "cpu_baseline"}
OUTPUTS = ["positions", "velocities", "thermostat_eta", "thermostat_eta_dot", "thermostat_kinetic_energies"]


def _bench(argv):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--molecules", "20000", "--steps", "40", "--warmup", "5"] + argv,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout.decode()
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_time_the_same_steps_and_dump_the_same_outputs(tmp_path):
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")])
    assert plain["steps"] == 40 and plain["value"] > 0 and plain["unit"] == "steps/s" and plain["higher_is_better"] is True
    assert plain["dtype"] == "f64" and abs(plain["ms_per_step"] - 1e3 / plain["value"]) <= 2e-3 * plain["ms_per_step"]
    assert not MOVED & set(plain)
    full = _bench(["--full", "--cpu-seconds", "1", "--dump-outputs", str(tmp_path / "full")])
    assert MOVED <= set(full) and full["steps"] == 40 and full["config"]["variant"] == plain["config"]["variant"]
    for name in OUTPUTS:
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a.dtype == np.float64 and a.size and np.all(np.isfinite(a)), name
        assert np.array_equal(a, b), name
    assert np.load(tmp_path / "plain" / "positions.npy").shape == (5 * 20000, 3)
