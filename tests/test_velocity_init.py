"""CPU side of tgnh_set_velocities_to_temperature / tgnh_set_temperatures: the yardstick of the GPU tests and what of the two
entry points a host-only handle can answer.

The yardstick is `draw` below: the specification in include/drude_tgnh.h (the comment above
tgnh_set_velocities_to_temperature) restated in numpy -- Philox4x32-10 on uint64 arrays, Box-Muller, the per-slot formulas from
the inverse masses velm holds (m = 1 / w, w = 1 / system.mass rounded once to velm's type, 0 for a massless slot) and the pair
lists.  It is written from that text, not from the kernel; tests/test_velocity_init_gpu.py imports it."""
import ctypes as C

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator, HostTopology

MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10; every argument a uint64 array (or scalar) holding one 32-bit word."""
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    c0, c1, c2, c3, k0, k1 = (np.asarray(x, np.uint64) for x in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                            # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + w0) & MASK, (k1 + w1) & MASK
    return c0, c1, c2, c3


def normals(seed, index):
    """z(i) [len(index), 3]: key = (low, high word of seed), counter = (low, high word of the global index, 0, 0)"""
    seed, index = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), np.asarray(index, np.uint64)
    zero = np.zeros_like(index)
    x = philox4x32_10(index & MASK, index >> S32, zero, zero, seed & MASK, seed >> S32)
    u0, u1, u2, u3 = ((w.astype(np.float64) + 0.5) * 2.0 ** -32 for w in x)
    r0, r1 = np.sqrt(-2.0 * np.log(u0)), np.sqrt(-2.0 * np.log(u2))
    return np.stack([r0 * np.cos(2.0 * np.pi * u1), r0 * np.sin(2.0 * np.pi * u1), r1 * np.cos(2.0 * np.pi * u3)], 1)


def inverse_masses(system, precision):
    """w as a context stores it: 1 / mass in fp64, rounded once to velm's type; 0 for a massless slot"""
    inv = np.where(system.mass == 0.0, 0.0, 1.0 / np.where(system.mass == 0.0, 1.0, system.mass))
    return inv.astype(np.float32).astype(np.float64) if precision == "single" else inv


def draw(w, pair_drude, pair_parent, temperature, drude_temperature, seed, first_particle=0, kB=synth.KB):
    """-> (v [n, 3] in fp64, sigma [n]: the slot's own sqrt(kB T / m), or the larger of its pair's two factors)"""
    n = len(w)
    z = normals(seed, np.uint64(first_particle) + np.arange(n, dtype=np.uint64))
    m = np.where(w != 0, 1.0 / np.where(w != 0, w, 1.0), 0.0)
    v, sigma = np.zeros((n, 3)), np.zeros(n)
    free = w != 0
    free[pair_drude] = False
    free[pair_parent] = False
    sigma[free] = np.sqrt(kB * temperature / m[free])
    v[free] = sigma[free, None] * z[free]
    md, mp = m[pair_drude], m[pair_parent]
    mt = md + mp
    mu = md * mp / mt
    scm, srel = np.sqrt(kB * temperature / mt), np.sqrt(kB * drude_temperature / mu)
    vcm, vrel = scm[:, None] * z[pair_parent], srel[:, None] * z[pair_drude]
    v[pair_drude] = vcm - vrel * (mp / mt)[:, None]
    v[pair_parent] = vcm + vrel * (md / mt)[:, None]
    sigma[pair_drude] = sigma[pair_parent] = np.maximum(scm, srel)
    return v, sigma


def thermostat_temperatures(system, v, dof, kB=synth.KB):
    """[group 0, COM, Drude] of a one-group TGNH handle with the COM group: the kinetic energies of K :138-200 (ordinary
    particles and pair centres of mass relative to their molecule's centre of mass | molecular centres of mass | the relative
    motion of the pairs with the reduced mass), each over its degrees of freedom and kB"""
    m = system.mass
    nres = system.num_residues
    mres = np.bincount(system.resid, m, nres)
    vcom = np.stack([np.bincount(system.resid, m * v[:, k], nres) for k in range(3)], 1) / mres[:, None]
    pd, pp = system.pair_drude, system.pair_parent
    free = m > 0
    free[pd] = False
    free[pp] = False
    ke_group = (m[free] * ((v[free] - vcom[system.resid[free]]) ** 2).sum(1)).sum()
    mt = m[pd] + m[pp]
    vcm = (m[pd, None] * v[pd] + m[pp, None] * v[pp]) / mt[:, None]
    ke_group += (mt * ((vcm - vcom[system.resid[pd]]) ** 2).sum(1)).sum()
    ke_com = (mres * (vcom ** 2).sum(1)).sum()
    ke_drude = (m[pd] * m[pp] / mt * ((v[pp] - v[pd]) ** 2).sum(1)).sum()
    return np.array([ke_group, ke_com, ke_drude]) / dof / kB


# The two seeds of the statistical test on the GPU (test_velocity_init_gpu.py): for each the yardstick alone puts every
# thermostat of water_box(4096) within 4 sqrt(2 / n_i) of its target (checked below), so the 5 sqrt(2 / n_i) asked of the device
# is not a coin toss
STAT_SEEDS = (20191024, 7)


def integ(temperature=300.0, drude_temperature=1.0, chains=3, drude_chains=True):
    return DrudeTGNHIntegrator(temperature, 0.1, drude_temperature, 0.005, 0.001, 20, chains, drude_chains, True)


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10 (kat_vectors)"""
    f = 0xFFFFFFFF
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((f, f, f, f), (f, f), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        assert tuple(int(x) for x in philox4x32_10(*ctr, *key)) == want


def test_the_restatement_is_deterministic_and_takes_its_words_as_specified():
    idx = np.arange(1000, dtype=np.uint64)
    a, b = normals(12345, idx), normals(12345, idx)
    assert a.tobytes() == b.tobytes() and np.isfinite(a).all()
    # z(i) is a function of the global index: a shard that starts at slot 300 draws the whole system's rows 300..
    assert normals(12345, idx[300:]).tobytes() == a[300:].tobytes()
    # the counter's and the key's words, straight through Philox
    x = philox4x32_10(5, 9, 0, 0, 3, 4)
    u = [(float(w) + 0.5) * 2.0 ** -32 for w in x]
    want = [np.sqrt(-2 * np.log(u[0])) * np.cos(2 * np.pi * u[1]), np.sqrt(-2 * np.log(u[0])) * np.sin(2 * np.pi * u[1]),
            np.sqrt(-2 * np.log(u[2])) * np.cos(2 * np.pi * u[3])]
    assert normals(3 + (4 << 32), np.array([5 + (9 << 32)], np.uint64))[0].tolist() == want
    # the seed's high word and an index above 2^32 change the output
    assert not np.array_equal(normals(3, idx[:8]), normals(3 + (1 << 32), idx[:8]))
    assert not np.array_equal(normals(3, idx[:8]), normals(3, idx[:8] + np.uint64(1 << 32)))
    # |z| stays below the 6.8 the tolerance of the GPU test is derived for: r <= sqrt(-2 ln 2^-33)
    assert np.sqrt(-2 * np.log(0.5 * 2.0 ** -32)) < 6.8


def test_the_draw_follows_synths_recipe():
    """massless 0, the pair decomposed with synth._finish's signs, zero temperature exact zeros, w's rounding taken"""
    s, _, _ = synth.pair_normal_massless()
    w = inverse_masses(s, "double")
    v, sigma = draw(w, s.pair_drude, s.pair_parent, 300.0, 1.0, 99)
    z = normals(99, np.arange(4))
    m = s.mass
    assert (v[3] == 0).all() and sigma[3] == 0
    np.testing.assert_allclose(v[2], np.sqrt(synth.KB * 300.0 / m[2]) * z[2], rtol=1e-15)
    mt = m[0] + m[1]
    np.testing.assert_allclose((m[0] * v[0] + m[1] * v[1]) / mt, np.sqrt(synth.KB * 300.0 / mt) * z[0], rtol=1e-13)      # centre of mass: z(parent) at T
    np.testing.assert_allclose(v[0] - v[1], np.sqrt(synth.KB * 1.0 * mt / (m[0] * m[1])) * z[1], rtol=1e-13)               # v_parent - v_drude: z(Drude) at T_D
    assert (draw(w, s.pair_drude, s.pair_parent, 0.0, 0.0, 99)[0] == 0).all()
    assert not np.array_equal(draw(inverse_masses(s, "single"), s.pair_drude, s.pair_parent, 300.0, 1.0, 99)[0], v)


@pytest.mark.parametrize("seed", STAT_SEEDS)
def test_temperatures_land_where_the_thermostats_look(seed):
    """chi^2 with n_i degrees of freedom per thermostat: relative sigma sqrt(2 / n_i).  The seeds named for the GPU test sit
    within 4 sigma in the yardstick alone."""
    s, _, _ = synth.water_box(4096)
    top = HostTopology(s, integ(), mode="TGNH")
    dof, _ = top.dof()
    top.close()
    np.testing.assert_allclose(dof, [6 * 4096, 3 * 4096, 3 * 4096], rtol=1e-12)
    v, _ = draw(inverse_masses(s, "mixed"), s.pair_drude, s.pair_parent, 300.0, 1.0, seed)
    t = thermostat_temperatures(s, v, dof)
    dev = np.abs(t / np.array([300.0, 300.0, 1.0]) - 1.0) / np.sqrt(2.0 / dof)
    print(f"seed {seed}: T = {t}, deviation in sigmas = {dev}")
    assert (dev <= 4.0).all(), (t, dev)


def test_argument_checks_through_a_host_only_handle():
    lib = _lib.load()
    s, _, _ = synth.nacl()
    top = HostTopology(s, integ(), mode="TGNH")
    call = lambda *a: lib.tgnh_set_velocities_to_temperature(*a)
    assert call(None, 300.0, 1.0, 1, 0, None) == _lib.ERR_ARG
    for t, td in ((-1.0, 1.0), (300.0, -1.0), (np.nan, 1.0), (300.0, np.nan), (np.inf, 1.0), (300.0, -np.inf)):
        assert call(top.h, t, td, 1, 0, None) == _lib.ERR_ARG, (t, td)
        assert lib.tgnh_set_temperatures(top.h, t, td, None) == _lib.ERR_ARG, (t, td)
    assert call(top.h, 300.0, 1.0, 1, -1, None) == _lib.ERR_ARG
    assert call(top.h, 300.0, 1.0, 1, 0, None) == _lib.ERR_STATE          # host-only: nothing launches
    assert call(top.h, 0.0, 0.0, -1, 2 ** 40, None) == _lib.ERR_STATE      # (legal values: the refusal is the handle's)
    assert b"host-only" in lib.tgnh_last_error()
    assert lib.tgnh_set_temperatures(None, 300.0, 1.0, None) == _lib.ERR_ARG
    top.close()


@pytest.mark.parametrize("mode,drude_chains", [("TGNH", True), ("dualNH", True), ("dualNH", False)])
def test_retargeting_gives_the_bookkeeping_of_a_handle_created_there(mode, drude_chains):
    """N kT (tgnh_get_dof) and the thermostat masses of a retargeted host-only handle are, bit for bit, those of a handle
    created at the new temperatures; eta, etaDot, etaDotDot stay what they were"""
    lib = _lib.load()
    s, _, _ = synth.nacl()
    a = HostTopology(s, integ(300.0, 1.0, 3, drude_chains), mode=mode)
    b = HostTopology(s, integ(350.0, 2.0, 3, drude_chains), mode=mode)
    before = [a.thermostat_state(k) for k in range(4)]
    assert not np.array_equal(a.dof()[1], b.dof()[1])
    assert lib.tgnh_set_temperatures(a.h, 350.0, 2.0, None) == _lib.TGNH_OK
    assert a.dof()[1].tobytes() == b.dof()[1].tobytes() and a.dof()[0].tobytes() == b.dof()[0].tobytes()
    assert a.thermostat_state(3).tobytes() == b.thermostat_state(3).tobytes()
    assert not np.array_equal(a.thermostat_state(3), before[3])
    for k in range(3):
        assert a.thermostat_state(k).tobytes() == before[k].tobytes()
    a.close()
    b.close()


def test_an_unbound_integrator_just_keeps_its_temperatures():
    it = integ()
    it.setTemperature(350)
    it.setDrudeTemperature(2)
    assert (it.getTemperature(), it.getDrudeTemperature()) == (350.0, 2.0)
