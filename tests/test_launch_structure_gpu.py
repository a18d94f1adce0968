"""The launch structure of the host step path, pinned: how many timed scopes of each kernel id (tgnh_timing_read) a fixed call
sequence produces, per handle configuration.  bench.py divides a kernel's time by these counts and every pass structure is
these launches in this order, so a change of the host orchestration that is meant to preserve behaviour must leave every row
of EXPECTED as it is; a change that is meant to move a row says so by editing it.

The rows are what the library gave before the step orchestration was rewritten (`python tests/test_launch_structure_gpu.py
--print`, with the repository root on PYTHONPATH, prints the table for the library it finds).  Each is ten steps, a thermostat
query after step 5, a velocity read-back after step 7, then one round of the split path.  Against DESIGN.md 3.1, "launches per
step", for unsharded water with one link:
  plain            KE, rescale+kick+drift, force, kick+KE, rescale per step; the row sums and the chain run inside the two
                   rescale launches: no chain_kernel launch, no KID_CHAIN scope (the split round: one more KE pass and rescale)
  trust            the same without the begin half's KE pass (the two that remain are the split round's)
  defer            rescale+kick+drift, force, kick+KE per step; a chain launch only where a query or a flush materialises one
  defer+resident   one KID_STEP scope per step_begin that finds an end half waiting (7 of 10: not the first, not after a query)
  resident         two KID_STEP scopes per step, one per thermostat half (and two in the split round)
"""
import functools

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import (DrudeTGNHIntegrator, HipContext, FLAG_DEFER_SCALE, FLAG_RESIDENT_STEP,
                                                   FLAG_WAVE_TILES, FLAG_TRUST_STATE_CHANGED)

pytestmark = pytest.mark.gpu

KIDS = (_lib.KID_SKD, _lib.KID_KICK_KE, _lib.KID_SCALE, _lib.KID_KE, _lib.KID_CHAIN, _lib.KID_FORCE, _lib.KID_OTHER, _lib.KID_STEP)


def _gather_water():
    from helpers import drudes_at_the_end
    return drudes_at_the_end(60)


# the smallest systems that reach each branch of the step path; (builder, extra flags)
SYSTEMS = {
    "water27": (lambda: synth.water_box(27), FLAG_WAVE_TILES),            # wave tiles (wke_kernel, its tail sum, wstep_kernel)
    "mixed": (lambda: synth.mixed(300, 20), 0),                           # 512-slot tiles
    "polymer": (lambda: synth.polymer_in_water(700, 300), 0),             # a molecule longer than a tile: run_big_com
    "groups12": (lambda: synth.many_groups(300, 20, 12), 0),              # more thermostats than CHAIN_INLINE_SUM_NT
    "gather": (_gather_water, 0),                                         # the gather path
}
FLAGS = {
    "plain": 0,
    "trust": FLAG_TRUST_STATE_CHANGED,
    "defer": FLAG_DEFER_SCALE,
    "defer+resident": FLAG_DEFER_SCALE | FLAG_RESIDENT_STEP,
    "resident": FLAG_RESIDENT_STEP,
}
CHAINS = (1, 3)
CASES = [(s, f, c, x) for s in SYSTEMS for f in FLAGS for c in CHAINS
         for x in ("none", "hook") + (("mailbox",) if s in ("water27", "mixed") else ())]


@functools.lru_cache(maxsize=None)
def _system(name):
    return SYSTEMS[name][0]()


def scope_counts(sysname, flagname, chains, exchange):
    """the eight scope counts of the fixed call sequence on a fresh handle"""
    s, g, ng = _system(sysname)
    it = DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, chains, True, True)
    it.setMaxDrudeDistance(0.02)
    for _ in range(ng):
        it.addTempGroup()
    it._particleTempGroup = np.ascontiguousarray(g, np.int32)
    ctx = HipContext(s, it, mode="TGNH", precision="mixed", flags=FLAGS[flagname] | SYSTEMS[sysname][1])
    try:
        if exchange == "hook":
            ctx.set_allreduce(lambda t: None)                # one rank: the sums are the total already
        elif exchange == "mailbox":                          # one rank, its own mailbox
            box = ctx.exchange_create(1, 0)[1]
            ctx.set_global_dof_terms(ctx.local_dof_terms())
            ctx.exchange_attach_pointers([box])
        ctx.torch.cuda.synchronize()
        ctx.timing(True)
        for k in range(1, 11):
            ctx.step(1)
            if k == 5:
                ctx.last_kinetic_energies()                  # materialize_chain (and settle_end) on the path
            if k == 7:
                ctx.getVelocities()                          # flush_impl
        st = ctx._stream
        for fn in (ctx.lib.tgnh_step_begin_kick, ctx.lib.tgnh_step_begin_move):
            assert fn(ctx.h, st()) == 0
        ctx.compute_forces()
        for fn in (ctx.lib.tgnh_step_end_kick, ctx.lib.tgnh_step_end_thermo):
            assert fn(ctx.h, st()) == 0
        ctx.torch.cuda.synchronize()
        ctx.timing(False)
        assert ctx.check() == 0
        return tuple(ctx.timing_read(k)[1] for k in KIDS)
    finally:
        if exchange == "mailbox":
            ctx.exchange_detach()
        ctx.close()


# (system, flags, links, exchange) -> scopes of (scale+kick+drift, kick+KE, rescale, KE, chain, force, other, resident step)
EXPECTED = {
    ('water27', 'plain', 1, 'none'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('water27', 'plain', 1, 'hook'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('water27', 'plain', 1, 'mailbox'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('water27', 'plain', 3, 'none'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('water27', 'plain', 3, 'hook'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('water27', 'plain', 3, 'mailbox'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('water27', 'trust', 1, 'none'): (10, 10, 11, 2, 0, 11, 3, 0),
    ('water27', 'trust', 1, 'hook'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('water27', 'trust', 1, 'mailbox'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('water27', 'trust', 3, 'none'): (10, 10, 11, 2, 0, 11, 3, 0),
    ('water27', 'trust', 3, 'hook'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('water27', 'trust', 3, 'mailbox'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('water27', 'defer', 1, 'none'): (10, 10, 2, 2, 3, 11, 3, 0),
    ('water27', 'defer', 1, 'hook'): (10, 10, 2, 2, 3, 11, 3, 0),
    ('water27', 'defer', 1, 'mailbox'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('water27', 'defer', 3, 'none'): (10, 10, 2, 2, 3, 11, 3, 0),
    ('water27', 'defer', 3, 'hook'): (10, 10, 2, 2, 3, 11, 3, 0),
    ('water27', 'defer', 3, 'mailbox'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('water27', 'defer+resident', 1, 'none'): (3, 3, 2, 2, 3, 11, 3, 7),
    ('water27', 'defer+resident', 1, 'hook'): (10, 10, 2, 2, 3, 11, 3, 0),
    ('water27', 'defer+resident', 1, 'mailbox'): (3, 3, 2, 2, 8, 11, 3, 7),
    ('water27', 'defer+resident', 3, 'none'): (3, 3, 2, 2, 3, 11, 3, 7),
    ('water27', 'defer+resident', 3, 'hook'): (10, 10, 2, 2, 3, 11, 3, 0),
    ('water27', 'defer+resident', 3, 'mailbox'): (3, 3, 2, 2, 8, 11, 3, 7),
    ('water27', 'resident', 1, 'none'): (0, 0, 0, 0, 0, 11, 2, 22),
    ('water27', 'resident', 1, 'hook'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('water27', 'resident', 1, 'mailbox'): (0, 0, 0, 0, 0, 11, 2, 22),
    ('water27', 'resident', 3, 'none'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('water27', 'resident', 3, 'hook'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('water27', 'resident', 3, 'mailbox'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('mixed', 'plain', 1, 'none'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('mixed', 'plain', 1, 'hook'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('mixed', 'plain', 1, 'mailbox'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('mixed', 'plain', 3, 'none'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('mixed', 'plain', 3, 'hook'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('mixed', 'plain', 3, 'mailbox'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('mixed', 'trust', 1, 'none'): (10, 10, 11, 2, 0, 11, 3, 0),
    ('mixed', 'trust', 1, 'hook'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('mixed', 'trust', 1, 'mailbox'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('mixed', 'trust', 3, 'none'): (10, 10, 11, 2, 0, 11, 3, 0),
    ('mixed', 'trust', 3, 'hook'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('mixed', 'trust', 3, 'mailbox'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('mixed', 'defer', 1, 'none'): (10, 10, 2, 2, 3, 11, 3, 0),
    ('mixed', 'defer', 1, 'hook'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('mixed', 'defer', 1, 'mailbox'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('mixed', 'defer', 3, 'none'): (10, 10, 2, 2, 3, 11, 3, 0),
    ('mixed', 'defer', 3, 'hook'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('mixed', 'defer', 3, 'mailbox'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('mixed', 'defer+resident', 1, 'none'): (3, 3, 2, 2, 3, 11, 3, 7),
    ('mixed', 'defer+resident', 1, 'hook'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('mixed', 'defer+resident', 1, 'mailbox'): (3, 3, 2, 2, 8, 11, 3, 7),
    ('mixed', 'defer+resident', 3, 'none'): (10, 10, 2, 2, 3, 11, 3, 0),
    ('mixed', 'defer+resident', 3, 'hook'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('mixed', 'defer+resident', 3, 'mailbox'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('mixed', 'resident', 1, 'none'): (0, 0, 0, 0, 0, 11, 2, 22),
    ('mixed', 'resident', 1, 'hook'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('mixed', 'resident', 1, 'mailbox'): (0, 0, 0, 0, 0, 11, 2, 22),
    ('mixed', 'resident', 3, 'none'): (10, 10, 11, 12, 0, 11, 3, 0),
    ('mixed', 'resident', 3, 'hook'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('mixed', 'resident', 3, 'mailbox'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('polymer', 'plain', 1, 'none'): (10, 10, 11, 12, 0, 11, 25, 0),
    ('polymer', 'plain', 1, 'hook'): (10, 10, 11, 12, 22, 11, 25, 0),
    ('polymer', 'plain', 3, 'none'): (10, 10, 11, 12, 0, 11, 25, 0),
    ('polymer', 'plain', 3, 'hook'): (10, 10, 11, 12, 22, 11, 25, 0),
    ('polymer', 'trust', 1, 'none'): (10, 10, 11, 2, 0, 11, 25, 0),
    ('polymer', 'trust', 1, 'hook'): (10, 10, 11, 12, 22, 11, 25, 0),
    ('polymer', 'trust', 3, 'none'): (10, 10, 11, 2, 0, 11, 25, 0),
    ('polymer', 'trust', 3, 'hook'): (10, 10, 11, 12, 22, 11, 25, 0),
    ('polymer', 'defer', 1, 'none'): (10, 10, 2, 2, 3, 11, 17, 0),
    ('polymer', 'defer', 1, 'hook'): (10, 10, 2, 2, 15, 11, 17, 0),
    ('polymer', 'defer', 3, 'none'): (10, 10, 2, 2, 3, 11, 17, 0),
    ('polymer', 'defer', 3, 'hook'): (10, 10, 2, 2, 15, 11, 17, 0),
    ('polymer', 'defer+resident', 1, 'none'): (3, 3, 2, 2, 3, 11, 17, 7),
    ('polymer', 'defer+resident', 1, 'hook'): (10, 10, 2, 2, 15, 11, 17, 0),
    ('polymer', 'defer+resident', 3, 'none'): (10, 10, 2, 2, 3, 11, 17, 0),
    ('polymer', 'defer+resident', 3, 'hook'): (10, 10, 2, 2, 15, 11, 17, 0),
    ('polymer', 'resident', 1, 'none'): (0, 0, 0, 0, 0, 11, 24, 22),
    ('polymer', 'resident', 1, 'hook'): (10, 10, 11, 12, 22, 11, 25, 0),
    ('polymer', 'resident', 3, 'none'): (10, 10, 11, 12, 0, 11, 25, 0),
    ('polymer', 'resident', 3, 'hook'): (10, 10, 11, 12, 22, 11, 25, 0),
    ('groups12', 'plain', 1, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('groups12', 'plain', 1, 'hook'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('groups12', 'plain', 3, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('groups12', 'plain', 3, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('groups12', 'trust', 1, 'none'): (10, 10, 11, 2, 12, 11, 3, 0),
    ('groups12', 'trust', 1, 'hook'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('groups12', 'trust', 3, 'none'): (10, 10, 11, 2, 22, 11, 3, 0),
    ('groups12', 'trust', 3, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('groups12', 'defer', 1, 'none'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('groups12', 'defer', 1, 'hook'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('groups12', 'defer', 3, 'none'): (10, 10, 2, 2, 12, 11, 3, 0),
    ('groups12', 'defer', 3, 'hook'): (10, 10, 2, 2, 24, 11, 3, 0),
    ('groups12', 'defer+resident', 1, 'none'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('groups12', 'defer+resident', 1, 'hook'): (10, 10, 2, 2, 15, 11, 3, 0),
    ('groups12', 'defer+resident', 3, 'none'): (10, 10, 2, 2, 12, 11, 3, 0),
    ('groups12', 'defer+resident', 3, 'hook'): (10, 10, 2, 2, 24, 11, 3, 0),
    ('groups12', 'resident', 1, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('groups12', 'resident', 1, 'hook'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('groups12', 'resident', 3, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('groups12', 'resident', 3, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('gather', 'plain', 1, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('gather', 'plain', 1, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('gather', 'plain', 3, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('gather', 'plain', 3, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('gather', 'trust', 1, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('gather', 'trust', 1, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('gather', 'trust', 3, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('gather', 'trust', 3, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('gather', 'defer', 1, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('gather', 'defer', 1, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('gather', 'defer', 3, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('gather', 'defer', 3, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('gather', 'defer+resident', 1, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('gather', 'defer+resident', 1, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('gather', 'defer+resident', 3, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('gather', 'defer+resident', 3, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('gather', 'resident', 1, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('gather', 'resident', 1, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
    ('gather', 'resident', 3, 'none'): (10, 10, 11, 12, 22, 11, 3, 0),
    ('gather', 'resident', 3, 'hook'): (10, 10, 11, 12, 44, 11, 3, 0),
}


@pytest.mark.parametrize("sysname,flagname,chains,exchange", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_timed_scopes_per_kernel_id(sysname, flagname, chains, exchange):
    got = scope_counts(sysname, flagname, chains, exchange)
    print(sysname, flagname, chains, exchange, got)
    assert got == EXPECTED[(sysname, flagname, chains, exchange)]


if __name__ == "__main__":
    import sys
    if "--print" in sys.argv:                            # (run with the repository root on PYTHONPATH)
        for case in CASES:
            print(f"    {case!r}: {scope_counts(*case)!r},", flush=True)
