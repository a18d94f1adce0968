"""tgnh_scale_velocities, tgnh_rescale_to_temperature, tgnh_get_rescale_factors, tgnh_set_velocity_rescaling without a GPU: the
factor rule of include/drude_tgnh.h restated in numpy, the identity the feature rests on checked with the oracle alone, the
argument checks through a host-only handle, the binding.  tests/test_velocity_rescale_gpu.py takes its systems, its integrator
and the factor rule from here.

The identity: with ke = kinetic_energies(v) and f_k = sqrt(target_k / ke_k), scale_velocities(v, f) leaves kinetic energies equal
to the targets -- the integrator's decomposition (A6) is orthogonal with respect to its own kinetic-energy bins (A3 / A4) as long as
no molecule spans two temperature groups.  The gate is the GPU file's for double precision, 1e-12 relative; measured here: at most
2.4e-15.  On the spanning system (water_box(27), every hydrogen in a second group) unequal factors inside a molecule move its
centre of mass and one application misses by 12 %: the GPU file compares that system with the oracle only.

drudes-at-the-end (every residue stored in two runs) with the COM group on is a second such case, and for a reason of the
reference's own: its centre-of-mass walk takes `count` consecutive particles from a residue's last run (K :90-91; library and
oracle follow it, tests/test_gather_gpu.py), so what it subtracts is not the molecule's centre of mass, the decomposition is not
orthogonal, and the oracle itself misses by more than 100 %.  Both files hold that system against the oracle with the COM group on
and off, and ask for the targets with the COM group off, where there is no walk."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator, HostTopology, KB, FLAG_DEFER_SCALE
from helpers import make_oracle, to_internal, drudes_at_the_end

MODES = ("TGNH", "dualNH")
T_NEW, TD_NEW = 350.0, 2.0
KE_GATE = {"double": 1e-12, "mixed": 1e-12, "single": 16 * 2.0 ** -24}


def spanning_water(n_mol=27):
    """a water box in which every molecule spans two temperature groups: O, its Drude and the M site in 0, the hydrogens in 1"""
    s, g, _ = synth.water_box(n_mol)
    g = g.copy()
    g[np.isin(np.arange(s.num_particles) % 5, (2, 3))] = 1      # (slots of a molecule: O, D, H1, H2, M)
    return s, g, 2


# the smallest shapes at which a stage can go wrong (tests/test_velocity_rescale_gpu.py says what each is for)
SYSTEMS = {"water1": lambda: synth.water_box(1),
           "water13": lambda: synth.water_box(13),
           "water300": lambda: synth.water_box(300),
           "nacl": synth.nacl,
           "ionic4": lambda: synth.ionic_liquid(4),
           "polymer": lambda: synth.polymer_in_water(300, 20),
           "groups40": lambda: synth.many_groups(60, 6, 40),
           "drudes-at-the-end": lambda: drudes_at_the_end(300),
           "water52": lambda: synth.water_box(52),
           "spanning": spanning_water}
ORACLE_ONLY = ("spanning",)
LANDS_WITHOUT_COM_ONLY = ("drudes-at-the-end",)             # (see the head of this file)
_cache = {}


def system(name):
    if name not in _cache:
        _cache[name] = SYSTEMS[name]()
    return _cache[name]


def plain_integrator(chains=3, com=True):
    return DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, chains, True, com)


def integ(name, mode, chains=3, com=True):
    """the integrator of a case, and the groups the oracle is given for it (dualNH knows no temperature groups)"""
    s, g, ng = system(name)
    it = plain_integrator(chains, com)
    if mode == "dualNH":
        return it, np.zeros_like(g), 1
    for _ in range(ng):
        it.addTempGroup()
    it._particleTempGroup = np.ascontiguousarray(g, np.int32)
    return it, g, ng


def to_oracle(x, mode):
    """the library's NT layout -> the oracle's thermostat vectors (dualNH: [real, Drude])"""
    x = np.asarray(x)
    return x[[0, 2]] if mode == "dualNH" else x


def targets(dof, temperature, drude_temperature, kB=KB):
    """N kT per thermostat at these temperatures, in the library's layout (the Drude bath is the last entry): kB T first, then the
    product with the degrees of freedom, as thermostat_nkt forms it"""
    t = np.asarray(dof, np.float64) * (kB * temperature)
    t[-1] = dof[-1] * (kB * drude_temperature)
    return t


def factor_rule(ke, target, inert):
    """include/drude_tgnh.h, tgnh_rescale_to_temperature: -> (factors, whether status bit 4 is raised)"""
    f, nan = np.ones(len(ke)), False
    for k in range(len(ke)):
        if inert[k]:
            continue
        if np.isnan(ke[k]):
            nan = True
        elif ke[k] > 0:
            f[k] = np.sqrt(np.float64(target[k]) / np.float64(ke[k]))
    return f, nan


# ---- 1. the factor rule
def test_the_factor_rule():
    ke = np.array([4.0, 0.0, 9.0, 7.0, 5.0, np.nan])
    target = np.array([16.0, 3.0, 0.0, 0.0, 10.0, 1.0])
    inert = np.array([False, False, False, True, False, False])
    f, nan = factor_rule(ke, target, inert)
    assert f[0] == 2.0                        # sqrt(16 / 4)
    assert f[1] == 1.0                        # no kinetic energy to scale
    assert f[2] == 0.0                        # a target of zero (a temperature of 0): a legal factor
    assert f[3] == 1.0                        # inert, whatever its sum
    assert f[4] == np.sqrt(2.0)
    assert f[5] == 1.0 and nan                # a NaN sum: factor 1, and the failure is reported
    assert not factor_rule(ke[:5], target[:5], inert[:5])[1]
    # one division, one square root, each rounded on its own
    a, b = np.float64(0.1), np.float64(0.3)
    assert factor_rule([b], [a], [False])[0][0] == np.sqrt(a / b)


# ---- 2. the identity, with the oracle alone
def landing_com(name):
    """the COM group of the cases that ask for the targets"""
    return name not in LANDS_WITHOUT_COM_ONLY


def scaled_once(name, mode, temperature=T_NEW, drude_temperature=TD_NEW, com=None):
    """-> (kinetic energies after one scaling to the targets, the targets, the factors), the oracle's vectors in the library's layout"""
    s, _, _ = system(name)
    it, g, ng = integ(name, mode, com=landing_com(name) if com is None else com)
    o = make_oracle(s, g, ng, mode, it)
    v = s.velocities.copy()
    ke = to_internal(o.kinetic_energies(v), mode)
    dof = to_internal(o.dof()[0], mode)
    want = targets(dof, temperature, drude_temperature)
    f, nan = factor_rule(ke, want, dof == 0)
    assert not nan
    o.scale_velocities(v, to_oracle(f, mode))
    return to_internal(o.kinetic_energies(v), mode), want, f


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [n for n in SYSTEMS if n not in ORACLE_ONLY])
def test_one_scaling_lands_on_the_targets(name, mode):
    ke, want, f = scaled_once(name, mode)
    live = want > 0
    assert live.any() and (f[~live] == 1.0).all()
    err = np.abs(ke[live] - want[live]) / want[live]
    print(f"{name} {mode}: {int(live.sum())} live thermostats, factors {f[live].min():.4f} .. {f[live].max():.4f}, max rel. miss {err.max():.2e}")
    assert err.max() <= KE_GATE["double"]


def test_a_molecule_that_spans_two_groups_misses():
    ke, want, f = scaled_once("spanning", "TGNH")
    miss = np.abs(ke - want) / want
    print(f"spanning water: factors {f}, rel. miss {miss}")
    assert miss.max() > 0.01
    # residues in two runs, the COM group on: the reference's walk (TGNH mode only: dualNH has no COM group)
    ke, want, f = scaled_once("drudes-at-the-end", "TGNH", com=True)
    miss = np.abs(ke - want) / want
    print(f"drudes-at-the-end, COM group on: factors {f}, rel. miss {miss}")
    assert miss.max() > 0.01
    # dualNH knows no groups: the same box lands
    ke, want, _ = scaled_once("spanning", "dualNH")
    live = want > 0
    assert (np.abs(ke[live] - want[live]) <= KE_GATE["double"] * want[live]).all()


# ---- 3. the entry points' argument checks (a host-only handle, no GPU)
@pytest.mark.parametrize("mode", MODES)
def test_argument_checks_through_a_host_only_handle(mode):
    lib = _lib.load()
    s, _, _ = system("nacl")
    top = HostTopology(s, integ("nacl", mode)[0], mode=mode)
    NT = top.num_thermostats()
    arr = lambda *v: (C.c_double * len(v))(*v)                  # noqa: E731
    good = arr(*np.linspace(0.5, 2.0, NT))
    out = arr(*[7.0] * NT)
    # a null handle
    assert lib.tgnh_scale_velocities(None, good, NT, None) == _lib.ERR_ARG
    assert lib.tgnh_rescale_to_temperature(None, 300.0, 1.0, None) == _lib.ERR_ARG
    assert lib.tgnh_get_rescale_factors(None, None, out) == _lib.ERR_ARG
    assert lib.tgnh_set_velocity_rescaling(None, 1, 300.0, 1.0) == _lib.ERR_ARG
    # arguments: answered before the handle's state is looked at
    assert lib.tgnh_scale_velocities(top.h, None, NT, None) == _lib.ERR_ARG
    for count in (0, NT - 1, NT + 1, -NT):
        assert lib.tgnh_scale_velocities(top.h, good, count, None) == _lib.ERR_ARG, count
    live = [k for k in range(NT) if not (mode == "dualNH" and k == 1)]
    for k in live:
        for v in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
            odd = arr(*np.ones(NT))
            odd[k] = v
            assert lib.tgnh_scale_velocities(top.h, odd, NT, None) == _lib.ERR_ARG, (k, v)
    for t, td in ((np.nan, 1.0), (300.0, np.nan), (-1.0, 1.0), (300.0, -1e-9), (np.inf, 1.0), (300.0, np.inf)):
        assert lib.tgnh_rescale_to_temperature(top.h, t, td, None) == _lib.ERR_ARG, (t, td)
        assert lib.tgnh_set_velocity_rescaling(top.h, 1, t, td) == _lib.ERR_ARG, (t, td)
    assert lib.tgnh_set_velocity_rescaling(top.h, -1, 300.0, 1.0) == _lib.ERR_ARG
    assert lib.tgnh_get_rescale_factors(top.h, None, None) == _lib.ERR_ARG
    # well-formed calls: the refusal is the handle's (device -1: nothing launches)
    assert lib.tgnh_scale_velocities(top.h, good, NT, None) == _lib.ERR_STATE
    assert lib.tgnh_scale_velocities(top.h, arr(*np.zeros(NT)), NT, None) == _lib.ERR_STATE        # 0 is a legal factor
    if mode == "dualNH":                                                                            # the unused entry is not looked at
        odd = arr(1.0, np.nan, 1.0)
        assert lib.tgnh_scale_velocities(top.h, odd, NT, None) == _lib.ERR_STATE
    assert lib.tgnh_rescale_to_temperature(top.h, 350.0, 2.0, None) == _lib.ERR_STATE
    assert lib.tgnh_rescale_to_temperature(top.h, 0.0, 0.0, None) == _lib.ERR_STATE                 # 0 is a legal temperature
    assert lib.tgnh_get_rescale_factors(top.h, None, out) == _lib.ERR_STATE
    assert list(out) == [7.0] * NT                                                                  # nothing was written
    # the setter only takes note
    for every in (0, 1, 3, 0):
        assert lib.tgnh_set_velocity_rescaling(top.h, every, 300.0, 1.0) == _lib.TGNH_OK
    # it leaves the baths alone
    assert np.array_equal(top.dof()[1], targets(top.dof()[0], 300.0, 1.0))
    top.close()


def test_the_setter_is_refused_on_a_deferred_handle():
    lib = _lib.load()
    s, _, _ = system("nacl")
    top = HostTopology(s, integ("nacl", "TGNH")[0], mode="TGNH", flags=FLAG_DEFER_SCALE)
    assert lib.tgnh_set_velocity_rescaling(top.h, 1, 300.0, 1.0) == _lib.ERR_UNSUPPORTED
    assert b"DEFER_SCALE" in lib.tgnh_last_error()
    assert lib.tgnh_set_velocity_rescaling(top.h, 0, 300.0, 1.0) == _lib.TGNH_OK      # off is what it is already
    assert lib.tgnh_set_velocity_rescaling(top.h, -1, 300.0, 1.0) == _lib.ERR_ARG
    top.close()


def test_the_targets_are_what_the_handle_would_report():
    """targets() above -- what both files compare kinetic energies with -- is tgnh_get_dof's N kT of a handle created at those
    temperatures, bit for bit"""
    for name in ("nacl", "groups40", "polymer"):
        for mode in MODES:
            s, _, _ = system(name)
            it, _, _ = integ(name, mode)
            it.setTemperature(T_NEW)
            it.setDrudeTemperature(TD_NEW)
            top = HostTopology(s, it, mode=mode)
            dof, nkt = top.dof()
            assert np.array_equal(nkt, targets(dof, T_NEW, TD_NEW)), (name, mode)
            top.close()


# ---- 4. the binding
def test_binding_signatures():
    S = _lib.SIGNATURES
    assert S["tgnh_scale_velocities"] == (C.c_int, [C.c_void_p, _lib.c_f64p, C.c_int, C.c_void_p])
    assert S["tgnh_rescale_to_temperature"] == (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_void_p])
    assert S["tgnh_get_rescale_factors"] == (C.c_int, [C.c_void_p, C.c_void_p, _lib.c_f64p])
    assert S["tgnh_set_velocity_rescaling"] == (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double])
    lib = _lib.load()
    for name in ("tgnh_scale_velocities", "tgnh_rescale_to_temperature", "tgnh_get_rescale_factors", "tgnh_set_velocity_rescaling"):
        assert getattr(lib, name).argtypes == S[name][1]
