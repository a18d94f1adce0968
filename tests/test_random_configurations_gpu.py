"""A fixed slice of tests/oracle_soak.py in the suite: the HIP path against the oracle over RANDOM configurations -- topology x mode x
precision x flag set x tile kind x chain length x every integrator parameter, the temperature groups handed over in both modes
(round 4: dualNH used them as bin indices; no test that zeroed them first could see it) -- and the same for the particle-sharded
path, two ranks on this GPU through the library's mailboxes.  The soak itself runs tens of thousands of such cases
(profiles/r04_fuzz_soak.md); these seeds are the suite's share."""
import numpy as np
import pytest

import oracle_soak

pytestmark = pytest.mark.gpu


STRUCTURAL = ("(an empty shard)", "(mailbox: <= 34 thermostats)")      # sharded_case's named skips: nothing to shard, or no mailbox for it


def _run(case, seeds, nsteps):
    """-> counts of four outcomes: ok; refused at create (TGNH_ERR_UNSUPPORTED: oracle_soak.REFUSED grows); no verdict from the
    oracle (OracleError: random constraint clusters its own SHAKE gives up on); a structural skip of the sharded case.  Any other
    skip is a failure."""
    verdicts = {"ok": 0, "refused": 0, "no_verdict": 0, "structural": 0}
    for seed in seeds:
        info = {"what": ""}
        refused = sum(oracle_soak.REFUSED.values())
        try:
            kind, what = case(np.random.default_rng(seed), nsteps, info)[:2]
        except oracle_soak.OracleError:
            kind, what = "no_verdict", ""
        except Exception as e:
            raise AssertionError(f"seed {seed}: {info['what']}") from e
        if kind == "skip":
            if sum(oracle_soak.REFUSED.values()) > refused:
                kind = "refused"
            elif what.endswith(STRUCTURAL):
                kind = "structural"
            else:
                raise AssertionError(f"seed {seed}: skipped for no named reason: {what}")
        verdicts[kind] += 1
    print(case.__name__, verdicts, dict(oracle_soak.REFUSED))
    return verdicts


def test_random_configurations_against_the_oracle():
    v = _run(oracle_soak.one_case, range(400), 30)
    assert v["refused"] == 0 and v["ok"] >= 388, v          # MI355X: 389 ok, 11 without a verdict from the oracle


def test_random_sharded_configurations_against_the_oracle():
    v = _run(oracle_soak.sharded_case, range(500000, 500150), 20)
    assert v["refused"] == 0 and v["ok"] >= 138, v          # MI355X: 139 ok, 11 structural skips


def test_random_checkpoints_restore_bit_for_bit():
    v = _run(oracle_soak.checkpoint_case, range(4000000, 4000150), 15)
    assert v["refused"] == 0 and v["ok"] >= 149, v          # MI355X: 150 of 150
