"""The hard wall's taken branch, on the CPU: the checks tests/test_hardwall_gpu.py rests on.

The GPU file compares every kernel form that carries a copy of the wall with helpers.hardwall_reference (np.longdouble, the
reference's two-member form) on constructed states (helpers.hot_wall_state).  A bounce is a discontinuity: a pair a rounding error
from the wall, from the deltaT clamp or from a sign change of a centred radial speed goes one way on the device and the other in
the reference without any bug.  So here, on the reference alone and for every case the GPU file runs:
  * the oracle's hard wall agrees with the independent fp80 restatement (and in the massless-parent branch, which the library
    refuses at create);
  * every class of pair is there (>= 3 pairs) in the begin that is compared, and every decision is >= 10 x the case's loosest
    tolerance from its threshold -- no pair has to be left out of any comparison;
  * each of six deliberate mis-restatements of the wall moves the result by > 100 x the tolerance: the GPU comparison would
    fail on a kernel that is wrong in that way.
"""
import numpy as np
import pytest

from openmm_drudenose_amd import synth
from oracle import Oracle, MODE_DUALNH, MODE_TGNH
from helpers import (HOT_DT, HOT_FORMS, HOT_KT_DRUDE, HOT_WALL, WALL_CLASSES, WALL_MUTANTS, HotCase, hardwall_reference, hot_form_cases,
                     hot_tolerances, hot_walls, rel_err, wall_classes, wall_margins)

# the reference-side cases behind the GPU file's: (system, mode, chains, delay, single precision among the runs?)
CASES = sorted({(s, m, c, HOT_FORMS[f]["delay"], p == "single") for f, s, m, c, p in hot_form_cases()})
IDS = ["-".join(map(str, c[:4])) + ("-single" if c[4] else "") for c in CASES]
_cache = {}


def case(sysname, mode, chains, delay, single):
    """(HotCase, walls, compared begins, reference steps, (tol_pos, tol_vel) of the loosest precision run on it), computed once"""
    key = (sysname, mode, chains, delay, single)
    if key not in _cache:
        hc = HotCase(sysname, mode, chains, delay)
        walls, compared = hot_walls(delay, "single" if single else "double")
        steps = hc.reference(walls)
        for st in steps:
            for a in st.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _cache[key] = (hc, walls, compared, steps, hot_tolerances("single" if single else "double", hc.kappa))
    return _cache[key]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_oracle_hardwall_agrees_with_the_fp80_restatement(c):
    """eps x kappa x a few operations: 2.2e-16 x 150 x 3 = 1e-13 bounds what fp64 can lose against fp80 in Drude - parent"""
    hc, walls, compared, steps, _ = case(*c)
    o = hc.oracle()
    for k in compared:
        pos, vel = steps[k]["pre_pos"].copy(), steps[k]["pre_vel"].copy()
        o.hardwall(pos, vel)
        ep, ev = rel_err(pos, steps[k]["pos"]), rel_err(vel, steps[k]["vel"])
        print(f"begin {k + 1}: oracle vs fp80 pos {ep:.1e} vel {ev:.1e}, {int(steps[k]['info']['out'].sum())} pairs bounced")
        assert ep <= 1e-13 and ev <= 1e-13


@pytest.mark.parametrize("mode", [MODE_TGNH, MODE_DUALNH])
def test_massless_parent_branch(mode):
    """Ref :323-334: only the Drude particle moves.  The library refuses a massless pair member at create; the oracle has the
    branch, and so has the fp80 restatement."""
    s = synth.DrudeSystem(mass=np.array([0.0, 0.4, 0.0, 0.4, 12.0]), pair_drude=np.array([1, 3]), pair_parent=np.array([0, 2]),
                          resid=np.zeros(5, np.int32), positions=np.array([[0, 0, 0], [0.0205, 0.001, 0], [1, 1, 1], [1, 1.001, 1.031], [2, 2, 2.0]]),
                          velocities=np.array([[0, 0, 0], [3.0, 1.0, -2.0], [0, 0, 0], [0.2, -0.1, -0.4], [0.1, 0.2, 0.3]]))
    o = Oracle(s, np.zeros(5, np.int32), 1, mode, 300.0, 0.1, 1.0, 0.005, HOT_DT, max_drude_distance=HOT_WALL, use_com_temp_group=False)
    pos, vel = s.positions.copy(), s.velocities.copy()
    o.hardwall(pos, vel)
    rp, rv, info = hardwall_reference(s.positions, s.velocities, s.mass, s.pair_drude, s.pair_parent, HOT_WALL, HOT_DT, HOT_KT_DRUDE)
    assert info["out"].all() and info["dt_raw"][0] < 1 < info["dt_raw"][1] and info["dotvr1"][1] < 0     # free; clamped and approaching
    assert np.array_equal(rp[[0, 2, 4]], s.positions[[0, 2, 4]]) and np.array_equal(rv[[0, 2, 4]], s.velocities[[0, 2, 4]])
    assert not np.array_equal(rp[[1, 3]], s.positions[[1, 3]])
    assert rel_err(pos, rp) <= 1e-15 and rel_err(vel, rv) <= 1e-15


# the classes a compared begin must hold.  The second begin of a state whose first begin had the wall too (delay = 0) is there for
# the late pairs, which cross in it (free, tangential); whatever else it holds (turned-round pairs just outside: clamped) is a
# kick's luck.  Nothing starts it 1.5 walls out or well outside and coming back: those classes are the first begin's, and the
# delayed states' second.
NEEDED = {(0, 0): WALL_CLASSES, (0, 1): ("inside", "free", "tangential"), (1, 1): WALL_CLASSES}


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_every_class_is_there_and_every_decision_has_margin(c):
    hc, walls, compared, steps, tol = case(*c)
    need = 10 * max(tol)
    for k in compared:
        info = steps[k]["info"]
        cl = wall_classes(info)
        m = wall_margins(info, np.abs(steps[k]["pre_vel"]).max())
        print(f"begin {k + 1}: " + " ".join(f"{n} {int(v.sum())}" for n, v in cl.items()) + " | margins " +
              " ".join(f"{n} {v:.1e}" for n, v in m.items()) + f" | needed {need:.1e}")
        assert (cl["inside"] ^ info["out"]).all() and (cl["free"] ^ cl["clamped"])[info["out"]].all()    # every pair is in a class: none is left out
        for name in NEEDED[(c[3], k)]:
            assert cl[name].sum() >= 3, (name, k)
        assert min(m.values()) >= need, m
        assert info["ratio"].max() < 2                                             # (the cases past twice the wall are their own test)


@pytest.mark.parametrize("mutant", WALL_MUTANTS)
@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_a_wrong_wall_would_be_seen(c, mutant):
    """In at least one compared begin the mutant's positions or velocities differ from the true reference's by more than 100 x the
    tolerance the GPU comparison applies to them."""
    hc, walls, compared, steps, tol = case(*c)
    wrong = hc.reference(walls, mutant=mutant)
    seen = []
    for k in compared:
        ep, ev = rel_err(wrong[k]["pos"], steps[k]["pos"]), rel_err(wrong[k]["vel"], steps[k]["vel"])
        seen.append((ep / tol[0], ev / tol[1]))
    print(mutant, " ".join(f"begin {k + 1}: pos {a:.1e} x tol, vel {b:.1e} x tol" for k, (a, b) in zip(compared, seen)))
    assert max(max(s) for s in seen) > 100


@pytest.mark.parametrize("mode", ["TGNH", "dualNH"])
@pytest.mark.parametrize("delay", [0, 1])
@pytest.mark.parametrize("what", ["beyond", "retargeted", "live"])
def test_the_further_gpu_cases_have_margin_too(what, delay, mode):
    """tests/test_hardwall_gpu.py's cases past twice the wall, at a Drude bath of 25 K and in a handle that has stepped before
    (all double precision, the 27-water box, one link): the same margins; past twice the wall, that pair alone and well past."""
    hc = HotCase("water27", mode, 1, delay, beyond=5 if what == "beyond" else None, drude_temperature=25.0 if what == "retargeted" else 1.0)
    walls, compared = hot_walls(delay, "double")
    steps = hc.reference(walls)
    for k in compared[:1] if what == "beyond" else compared:
        info = steps[k]["info"]
        m = wall_margins(info, np.abs(steps[k]["pre_vel"]).max())
        print(f"begin {k + 1}: {int(info['out'].sum())} bounced, margins " + " ".join(f"{n} {v:.1e}" for n, v in m.items()))
        assert info["out"].sum() >= 3 and min(m.values()) >= 10 * 1e-12
        if what == "beyond":
            assert info["ratio"][5] > 2.2 and np.delete(info["ratio"], 5).max() < 1.9
        else:
            assert info["ratio"].max() < 2


def test_wide_pairs_is_one_tile_and_far_pairs_is_none():
    """wide_pairs: partner and self 250-289 slots apart -- other wavefronts of the work-group -- and still on the tiled path;
    far_pairs: on the gather path by its topology."""
    from openmm_drudenose_amd.drudetgnhplugin import HostTopology
    from helpers import far_pairs, wide_pairs
    s = wide_pairs()[0]
    gap = np.abs(s.pair_drude - s.pair_parent)[-40:]
    assert gap.min() >= 250 and gap.max() <= 289 and s.num_particles <= 512
    hc = HotCase("wide", "TGNH", 1, 0)
    assert HostTopology(s, hc.make_integrator(HOT_WALL)).step_path() == ("tiled", "")
    hc = HotCase("far", "TGNH", 1, 0)
    path, why = HostTopology(far_pairs()[0], hc.make_integrator(HOT_WALL)).step_path()
    assert path == "gather" and "asked for" not in why
