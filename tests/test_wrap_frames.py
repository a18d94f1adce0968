"""CPU tests of the periodic box, tgnh_wrap_molecules / tgnh_write_frame's yardstick and argument checks, and reporters.DCDReporter.

`wrapped` and `frame_of` restate include/drude_tgnh.h's formulas in numpy on top of `centroids` of tests/test_scale_positions.py (a
molecule's sum taken member by member in ascending slot order, every partial sum rounded): c = S / n, then
    kz = floor(c_z / cz);            d = (kz cx, kz cy, kz cz)
    ky = floor((c_y - d_y) / by);    d_x = d_x + ky bx;   d_y = d_y + ky by
    kx = floor((c_x - d_x) / ax);    d_x = d_x + kx ax
each operation rounded on its own (numpy fuses nothing), x' = x - d for a molecule with a cell index that is not zero, nothing at all
for the others.  They are what tests/test_wrap_frames_gpu.py holds the kernels against, BIT FOR BIT: cell indices are integers and d
is formed from them and the box alone, so once a centroid falls in the same cell every stored value is the yardstick's -- also for
molecules of more than 64 members, whose sum the kernel takes in another order.  That rests on one condition, asserted here for
every case the GPU tests use: no centroid's fractional coordinate lies within 1e-4 of an integer, while two orders of n additions
move it by less than n 2^-52 sum|x| / n / L (below 6e-9 here)."""
import ctypes as C
import io
import struct

import numpy as np
import pytest

from openmm_drudenose_amd import synth, _lib
from openmm_drudenose_amd.drudetgnhplugin import DrudeTGNHIntegrator, HostTopology, TgnhError, FLAG_GATHER
from openmm_drudenose_amd.reporters import DCDReporter, cell_lengths_and_angles
from test_scale_positions import centroids, renumbered, coordinates, stored, arrays, REAL, StandIn
from test_scale_positions_gpu import CASES, case

WSHIFT = np.array([-0.47, -0.53, -0.37])                    # nm
BOX = np.array([[0.83, 0.0, 0.0], [0.17, 0.71, 0.0], [-0.29, 0.23, 0.97]])   # triclinic, incommensurate with the 0.31 nm lattice
WRAP, SKIP_DRUDE, INTERLEAVED = _lib.FRAME_WRAP, _lib.FRAME_SKIP_DRUDE, _lib.FRAME_INTERLEAVED
MARGIN = 1e-4


# ---- the yardstick ----
def shifts(c, box):
    """centroids [M, 3], box vectors [3, 3] -> (d [M, 3], moved [M], cell indices [M, 3] as (kx, ky, kz), fractional coordinates
    [M, 3] as the three floors saw them)"""
    box = np.asarray(box, np.float64)
    ax, bx, by, cx, cy, cz = box[0, 0], box[1, 0], box[1, 1], box[2, 0], box[2, 1], box[2, 2]
    with np.errstate(all="ignore"):
        fz = c[:, 2] / cz
        kz = np.floor(fz)
        dx, dy, dz = kz * cx, kz * cy, kz * cz
        fy = (c[:, 1] - dy) / by
        ky = np.floor(fy)
        dx, dy = dx + ky * bx, dy + ky * by
        fx = (c[:, 0] - dx) / ax
        kx = np.floor(fx)
        dx = dx + kx * ax
    moved = np.isfinite(c).all(1) & ((kx != 0) | (ky != 0) | (kz != 0))
    d = np.stack([dx, dy, dz], 1)
    d[~moved] = 0.0
    return d, moved, np.stack([kx, ky, kz], 1), np.stack([fx, fy, fz], 1)


def wrapped(pos_arrays, labels, box, precision):
    """include/drude_tgnh.h, tgnh_wrap_molecules, restated.  pos_arrays = (posq [N, 4], posq_correction [N, 4] or None) in their stored
    types -> the same pair after the wrap; molecules that stay, and w of both arrays, bit for bit."""
    posq, corr = pos_arrays
    posq = np.asarray(posq)
    assert posq.dtype == REAL[precision] and posq.shape[1] == 4 and (corr is not None) == (precision == "mixed")
    mol = renumbered(labels)
    x = coordinates(posq, corr)
    d, moved, _, _ = shifts(centroids(x, mol)[1], box)
    hi, lo = stored(x - d[mol], precision)
    sel = moved[mol]
    out, out_corr = posq.copy(), None
    out[sel, :3] = hi[sel]
    if corr is not None:
        out_corr = np.asarray(corr).copy()
        out_corr[sel, :3] = lo[sel]
    return out, out_corr


def frame_of(pos_arrays, labels, drude_slots, box, flags, unit, precision):
    """include/drude_tgnh.h, tgnh_write_frame, restated -> float32 [count, 3]: row j is output index j (the layout is the caller's)"""
    posq, corr = pos_arrays
    assert np.asarray(posq).dtype == REAL[precision]
    x = coordinates(posq, corr)
    d = np.zeros_like(x)
    if flags & WRAP:
        mol = renumbered(labels)
        d = shifts(centroids(x, mol)[1], box)[0][mol]
    keep = np.ones(len(x), bool)
    if flags & SKIP_DRUDE:
        keep[np.asarray(drude_slots, np.int64)] = False
    with np.errstate(over="ignore"):
        return (((x - d) * np.float64(unit)).astype(np.float32))[keep]


def inputs(name, precision):
    """(posq, corr) of a case of test_scale_positions_gpu.CASES for these tests, in the stored types: the system's positions + WSHIFT,
    charges in posq.w; in mixed precision 2^-12 is added to posq_correction.x of every slot of every second molecule, so that the
    split there is not the canonical one and a kernel that rewrites a molecule it should leave alone is caught."""
    s, labels, _ = case(name)
    rng = np.random.default_rng(5)
    posq, corr = arrays(s.positions + WSHIFT, rng.uniform(-1.0, 1.0, s.num_particles), precision)
    if corr is not None:
        odd = renumbered(labels) % 2 == 1
        corr[odd, 0] = corr[odd, 0] + np.float32(2.0 ** -12)
    return posq, corr


def integ(chains=3):
    return DrudeTGNHIntegrator(300.0, 0.1, 1.0, 0.005, 0.001, 20, chains, True, True)


# ---- 1. the yardstick's own checks ----
def test_the_yardstick_against_a_plain_loop():
    """synth.nacl(): every centroid within 2^-52 sum|x| of a plain long-double loop, and the cell indices of the two equal"""
    s, _, _ = synth.nacl()
    x = s.positions + WSHIFT
    mol = renumbered(s.resid)
    S, c, n, A = centroids(x, mol)
    d, moved, k, _ = shifts(c, BOX)
    L = np.longdouble
    for m in range(len(n)):
        acc = np.zeros(3, L)
        for i in np.flatnonzero(mol == m):
            acc = acc + x[i].astype(L)
        e = acc / L(n[m])
        assert (np.abs(c[m].astype(L) - e) <= 2.0 ** -52 * A[m]).all(), m
        kz = np.floor(e[2] / L(BOX[2, 2]))
        ky = np.floor((e[1] - kz * L(BOX[2, 1])) / L(BOX[1, 1]))
        kx = np.floor((e[0] - kz * L(BOX[2, 0]) - ky * L(BOX[1, 0])) / L(BOX[0, 0]))
        assert [float(kx), float(ky), float(kz)] == k[m].tolist(), m
        assert moved[m] == bool(kx or ky or kz)
    # ... and the move itself: x - x' is the molecule's d, every moved centroid lands in the cell
    out, _ = wrapped(arrays(x, np.zeros(len(x)), "double"), s.resid, BOX, "double")
    assert np.array_equal(out[:, :3], x - d[mol])
    _, again, k2, _ = shifts(centroids(out[:, :3], mol)[1], BOX)
    assert not again.any() and not k2.any()


@pytest.mark.parametrize("precision", ["double", "mixed", "single"])
def test_by_hand(precision):
    """powers of two and the box diag(2, 4, 8): every step exact in every type"""
    box = np.diag([2.0, 4.0, 8.0])
    #            on a face: c = L        just below zero                inside             a molecule of two, centre (3, 1, -4)
    x = np.array([[2.0, 4.0, 8.0], [-2.0 ** -60, 1.0, 1.0], [1.0, 2.0, 4.0], [2.5, 0.5, -3.5], [3.5, 1.5, -4.5]])
    labels = [4, 9, 1, 7, 7]
    posq, corr = arrays(x, [0.5, -1.0, 0.25, 2.0, 1.0], precision)
    if corr is not None:
        posq[2, 0], corr[2, 0] = 0.5, 0.5                       # the unmoved molecule: hi + lo = 1, a split no store would choose
    mol = renumbered(labels)
    d, moved, k, _ = shifts(centroids(coordinates(posq, corr), mol)[1], box)
    assert k.tolist() == [[1, 1, 1], [-1, 0, 0], [0, 0, 0], [1, 0, -1]]          # (-2^-60 is stored as it is in float32 too)
    assert moved.tolist() == [True, True, False, True] and d.tolist() == [[2, 4, 8], [-2, 0, 0], [0, 0, 0], [2, 0, -8]]
    out, out_corr = wrapped((posq, corr), labels, box, precision)
    assert out.dtype == posq.dtype and out[:, 3].tobytes() == posq[:, 3].tobytes()
    assert out[0, :3].tolist() == [0.0, 0.0, 0.0]               # c = L gives k = 1: it lands on 0
    assert out[1, :3].tolist() == [2.0, 1.0, 1.0]               # -2^-60 + 2 rounds to 2 in every type
    assert out[3:, :3].tolist() == [[0.5, 0.5, 4.5], [1.5, 1.5, 3.5]]
    assert out[2].tobytes() == posq[2].tobytes()                # the same bytes
    if corr is not None:
        assert out_corr[2].tobytes() == corr[2].tobytes() and out_corr[:, 3].tobytes() == corr[:, 3].tobytes()
        assert not out_corr[[0, 1, 3, 4], :3].any()
    f = frame_of((posq, corr), labels, [4], box, WRAP | SKIP_DRUDE, 4.0, precision)
    assert f.dtype == np.float32 and f.tolist() == [[0, 0, 0], [8, 4, 4], [4, 8, 16], [2, 2, 18]]
    f = frame_of((posq, corr), labels, [4], box, 0, 1.0, precision)
    assert f.shape == (5, 3) and np.array_equal(f, coordinates(posq, corr).astype(np.float32))


def test_by_hand_triclinic():
    """kz changes the x cell: c = (0.5, 1, 9) in a = (2, 0, 0), b = (0, 4, 0), c = (1, 0, 8) -- kz = 1 takes (1, 0, 8) off, and
    0.5 - 1 lies in the cell to the left"""
    box = np.array([[2.0, 0.0, 0.0], [0.0, 4.0, 0.0], [1.0, 0.0, 8.0]])
    x = np.array([[0.5, 1.0, 9.0]])
    d, moved, k, _ = shifts(x, box)
    assert k.tolist() == [[-1, 0, 1]] and d.tolist() == [[-1.0, 0.0, 8.0]] and moved.all()
    out, _ = wrapped(arrays(x, [0.0], "double"), [0], box, "double")
    assert out[0, :3].tolist() == [1.5, 1.0, 1.0]
    # a centroid that is not finite stays
    x = np.array([[np.nan, 1.0, 9.0], [0.5, np.inf, 9.0]])
    d, moved, _, _ = shifts(x, box)
    assert not moved.any() and not d.any()


# ---- 2. coverage of the inputs the GPU tests use ----
UNMOVED = {"water52": 4, "nacl": 18, "drudes-at-the-end": 18, "water52430": 18}


@pytest.mark.parametrize("name,precision", [(n, p) for n, (_, ps) in CASES.items() for p in ps])
def test_the_inputs_cover_both_branches_with_a_margin(name, precision):
    s, labels, _ = case(name)
    mol = renumbered(labels)
    x = coordinates(*inputs(name, precision))
    S, c, n, A = centroids(x, mol)
    d, moved, k, f = shifts(c, BOX)
    margin = np.abs(f - np.rint(f)).min()
    order = (n[:, None] * 2.0 ** -52 * A / n[:, None] / np.array([BOX[0, 0], BOX[1, 1], BOX[2, 2]]))[n > 64]
    print(f"{name} {precision}: margin {margin:.3e}, summation bound {order.max() if len(order) else 0.0:.3e}, "
          f"{int((~moved).sum())} of {len(n)} molecules stay, cells {k.min(0).tolist()} .. {k.max(0).tolist()}")
    assert margin >= MARGIN
    assert not len(order) or order.max() < 6e-9
    assert moved.any()
    if name in UNMOVED:                                          # (the small boxes lie in one corner of the cell's neighbourhood: all of theirs move)
        assert int((~moved).sum()) == UNMOVED[name]
    if name == "nacl":
        assert k.min(0).tolist() == [-2, -2, -1] and k.max(0).tolist() == [2, 2, 3]
    if precision == "mixed" and name in UNMOVED:                 # some molecule that stays carries the split no store would choose
        posq, corr = inputs(name, precision)
        hi, lo = stored(x, "mixed")
        odd = (corr[:, :3] != lo).any(1)
        assert (odd & ~moved[mol]).any() and (odd & moved[mol]).any()


# ---- 3. through a host-only handle ----
def vec(*v):
    return (C.c_double * 3)(*v)


def get_box(lib, h):
    a, b, c = vec(0, 0, 0), vec(0, 0, 0), vec(0, 0, 0)
    rc = lib.tgnh_get_periodic_box(h, a, b, c)
    return rc, [list(a), list(b), list(c)]


def test_the_box_through_a_host_only_handle():
    lib = _lib.load()
    top = HostTopology(synth.water_box(4)[0], integ())
    assert top.getPeriodicBoxVectors() is None
    assert get_box(lib, top.h)[0] == _lib.ERR_STATE
    top.setPeriodicBoxVectors(*BOX)
    rc, got = get_box(lib, top.h)
    assert rc == _lib.TGNH_OK and np.array(got).tobytes() == BOX.tobytes()              # bit for bit
    assert top.getPeriodicBoxVectors().tobytes() == BOX.tobytes()
    bad = {"ay": ((1, 1e-300, 0), (0, 1, 0), (0, 0, 1)), "az": ((1, 0, -0.1), (0, 1, 0), (0, 0, 1)), "bz": ((1, 0, 0), (0, 1, 0.1), (0, 0, 1)),
           "ax = 0": ((0, 0, 0), (0, 1, 0), (0, 0, 1)), "ax < 0": ((-1, 0, 0), (0, 1, 0), (0, 0, 1)), "by = 0": ((1, 0, 0), (0, 0, 0), (0, 0, 1)),
           "by < 0": ((1, 0, 0), (0, -1, 0), (0, 0, 1)), "cz = 0": ((1, 0, 0), (0, 1, 0), (0, 0, 0)), "cz < 0": ((1, 0, 0), (0, 1, 0), (0, 0, -1)),
           "bx": ((1, 0, 0), (0.51, 1, 0), (0, 0, 1)), "-bx": ((1, 0, 0), (-0.51, 1, 0), (0, 0, 1)), "cx": ((1, 0, 0), (0, 1, 0), (0.51, 0, 1)),
           "-cx": ((1, 0, 0), (0, 1, 0), (-0.51, 0, 1)), "cy": ((1, 0, 0), (0, 1, 0), (0, 0.51, 1)), "-cy": ((1, 0, 0), (0, 1, 0), (0, -0.51, 1))}
    for k in range(9):
        for v in (np.nan, np.inf, -np.inf):
            m = np.array(BOX)
            m.flat[k] = v
            bad[f"component {k} = {v}"] = m
    for what, m in bad.items():
        assert lib.tgnh_set_periodic_box(top.h, vec(*m[0]), vec(*m[1]), vec(*m[2])) == _lib.ERR_ARG, what
        assert np.array(get_box(lib, top.h)[1]).tobytes() == BOX.tobytes(), what       # the old box stays
    edge = ((1, 0, 0), (0.5, 1, 0), (-0.5, 0.5, 1))                                       # the bounds themselves are allowed
    assert lib.tgnh_set_periodic_box(top.h, vec(*edge[0]), vec(*edge[1]), vec(*edge[2])) == _lib.TGNH_OK
    assert get_box(lib, top.h)[1] == [list(map(float, r)) for r in edge]
    assert lib.tgnh_set_periodic_box(None, vec(*BOX[0]), vec(*BOX[1]), vec(*BOX[2])) == _lib.ERR_ARG
    assert lib.tgnh_set_periodic_box(top.h, None, vec(*BOX[1]), vec(*BOX[2])) == _lib.ERR_ARG
    assert lib.tgnh_get_periodic_box(top.h, None, None, None) == _lib.ERR_ARG
    with pytest.raises(TgnhError):
        top.setPeriodicBoxVectors((1, 0), (0, 1, 0), (0, 0, 1))
    top.close()


def test_the_frame_count_through_a_host_only_handle():
    lib = _lib.load()
    s, _, _ = synth.nacl()
    top = HostTopology(s, integ())
    n = C.c_int64(-1)
    assert top.frame_count() == 2500 and top.frame_count(skip_drude=True) == 2500 - 512
    for flags, want in ((0, 2500), (WRAP | INTERLEAVED, 2500), (SKIP_DRUDE, 1988), (WRAP | SKIP_DRUDE | INTERLEAVED, 1988)):
        assert lib.tgnh_get_frame_count(top.h, flags, C.byref(n)) == _lib.TGNH_OK and n.value == want
    n.value = -1
    assert lib.tgnh_get_frame_count(top.h, 8, C.byref(n)) == _lib.ERR_ARG and lib.tgnh_get_frame_count(top.h, -1, C.byref(n)) == _lib.ERR_ARG
    assert n.value == -1
    assert lib.tgnh_get_frame_count(top.h, 0, None) == _lib.ERR_ARG and lib.tgnh_get_frame_count(None, 0, C.byref(n)) == _lib.ERR_ARG
    top.close()


def desc(flags, count, unit=1.0, stride=None, capacity=None):
    d = _lib.TgnhFrameDesc()
    d.struct_size, d.flags, d.unit = C.sizeof(d), flags, unit
    d.stride = (0 if flags & INTERLEAVED else count) if stride is None else stride
    d.capacity = (3 * count if flags & INTERLEAVED else 2 * d.stride + count) if capacity is None else capacity
    return d


def test_argument_checks_through_a_host_only_handle():
    """the argument errors first, then TGNH_ERR_STATE: no box, and with one "host-only"""
    lib = _lib.load()
    s, _, _ = synth.nacl()
    top = HostTopology(s, integ(), flags=FLAG_GATHER)
    out = C.c_void_p(4096)                                      # (never dereferenced: nothing launches on this handle)
    N, K = 2500, 1988
    assert lib.tgnh_wrap_molecules(None, None) == _lib.ERR_ARG
    assert lib.tgnh_wrap_molecules(top.h, None) == _lib.ERR_STATE and b"box" in lib.tgnh_last_error()
    write = lambda d, o=out: lib.tgnh_write_frame(top.h, C.byref(d) if d is not None else None, o, None)    # noqa: E731
    assert lib.tgnh_write_frame(None, C.byref(desc(0, N)), out, None) == _lib.ERR_ARG
    assert write(None) == _lib.ERR_ARG and write(desc(0, N), None) == _lib.ERR_ARG
    d = desc(0, N); d.struct_size -= 4
    assert write(d) == _lib.ERR_ARG
    assert write(desc(8, N)) == _lib.ERR_ARG and write(desc(-2, N)) == _lib.ERR_ARG
    for unit in (0.0, -1.0, np.nan, np.inf, -np.inf):
        assert write(desc(0, N, unit=unit)) == _lib.ERR_ARG, unit
    assert write(desc(0, N, stride=N - 1, capacity=10 * N)) == _lib.ERR_ARG
    assert write(desc(SKIP_DRUDE, K, stride=K - 1, capacity=10 * N)) == _lib.ERR_ARG
    assert write(desc(INTERLEAVED, N, stride=N)) == _lib.ERR_ARG and write(desc(INTERLEAVED, N, stride=1)) == _lib.ERR_ARG
    assert write(desc(0, N, capacity=3 * N - 1)) == _lib.ERR_ARG
    assert write(desc(0, N, stride=N + 7, capacity=3 * N + 13)) == _lib.ERR_ARG
    assert write(desc(INTERLEAVED, N, capacity=3 * N - 1)) == _lib.ERR_ARG
    assert write(desc(SKIP_DRUDE | INTERLEAVED, K, capacity=3 * K - 1)) == _lib.ERR_ARG
    assert b"capacity" in lib.tgnh_last_error()
    # legal arguments: the refusal is the handle's
    assert write(desc(WRAP, N)) == _lib.ERR_STATE and b"box" in lib.tgnh_last_error()
    for flags, count in ((0, N), (SKIP_DRUDE, K), (INTERLEAVED, N), (SKIP_DRUDE | INTERLEAVED, K), (0, N)):
        assert write(desc(flags, count, unit=10.0)) == _lib.ERR_STATE and b"host-only" in lib.tgnh_last_error(), flags
    top.setPeriodicBoxVectors(*BOX)
    assert write(desc(WRAP | SKIP_DRUDE, K, stride=K + 7)) == _lib.ERR_STATE and b"host-only" in lib.tgnh_last_error()
    assert write(desc(WRAP, N, capacity=3 * N - 1)) == _lib.ERR_ARG                      # still the arguments first
    assert lib.tgnh_wrap_molecules(top.h, None) == _lib.ERR_STATE and b"host-only" in lib.tgnh_last_error()
    top.close()


def test_the_binding_declares_the_new_entry_points():
    S = _lib.SIGNATURES
    f64 = _lib.c_f64p
    assert S["tgnh_set_periodic_box"] == (C.c_int, [C.c_void_p, f64, f64, f64]) == S["tgnh_get_periodic_box"]
    assert S["tgnh_wrap_molecules"] == (C.c_int, [C.c_void_p, C.c_void_p])
    assert S["tgnh_get_frame_count"] == (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)])
    assert S["tgnh_write_frame"] == (C.c_int, [C.c_void_p] * 4)
    assert C.sizeof(_lib.TgnhFrameDesc) == 32 and _lib.TgnhFrameDesc.unit.offset == 8 and _lib.TgnhFrameDesc.capacity.offset == 24
    header = open(_lib.os.path.join(_lib.HERE, "..", "include", "drude_tgnh.h")).read()
    for name in ("tgnh_set_periodic_box", "tgnh_get_periodic_box", "tgnh_wrap_molecules", "tgnh_get_frame_count", "tgnh_write_frame"):
        assert f"tgnh_status {name}(" in header
    assert "enum { TGNH_FRAME_WRAP = 1, TGNH_FRAME_SKIP_DRUDE = 2, TGNH_FRAME_INTERLEAVED = 4 };" in header
    assert (WRAP, SKIP_DRUDE, INTERLEAVED) == (1, 2, 4)


# ---- 4. the reporter against a numpy stand-in ----
class FrameStandIn(StandIn):
    """StandIn with what DCDReporter uses: frame, frame_count, getPeriodicBoxVectors, time -- on numpy arrays through `frame_of`"""

    def __init__(self, positions, charges, labels, drude_slots, precision="double", box=None):
        super().__init__(positions, charges, labels, precision)
        self.drude_slots, self.box, self.steps, self.asked = np.asarray(drude_slots), box, 0, []

    def getPeriodicBoxVectors(self):
        return None if self.box is None else np.array(self.box)

    def frame_count(self, skip_drude=False):
        return len(self.posq) - (len(self.drude_slots) if skip_drude else 0)

    def time(self):
        return 0.001 * self.steps, self.steps

    def frame(self, wrap=False, skip_drude=False, unit=1.0, planes=False, out=None):
        flags = (WRAP if wrap else 0) | (SKIP_DRUDE if skip_drude else 0)
        self.asked.append((wrap, skip_drude, unit, planes))
        f = frame_of((self.posq, self.corr), self.labels, self.drude_slots, self.box, flags, unit, self.precision)
        return np.ascontiguousarray(f.T) if planes else f


def parse_dcd(raw, cell):
    """the file by the layout of reporters.py's docstring -> (header fields, [(cell doubles or None, planes [3, NATOM])])"""
    i32 = lambda at: struct.unpack_from("<i", raw, at)[0]        # noqa: E731
    assert i32(0) == 84 and raw[4:8] == b"CORD" and i32(88) == 84
    nset, istart, nsavc = struct.unpack_from("<3i", raw, 8)
    rest = struct.unpack_from("<6i", raw, 20)
    delta = struct.unpack_from("<f", raw, 44)[0]
    tail = struct.unpack_from("<10i", raw, 48)
    assert tail == (int(cell),) + (0,) * 8 + (24,)
    assert i32(92) == 164 and i32(96) == 2 and i32(100 + 160) == 164
    assert i32(264) == 4 and i32(272) == 4
    natom = i32(268)
    at, frames = 276, []
    while at < len(raw):
        box = None
        if cell:
            assert i32(at) == 48 and i32(at + 52) == 48
            box = struct.unpack_from("<6d", raw, at + 4)
            at += 56
        planes = []
        for _ in range(3):
            assert i32(at) == 4 * natom and i32(at + 4 + 4 * natom) == 4 * natom
            planes.append(np.frombuffer(raw, "<f4", natom, at + 4))
            at += 8 + 4 * natom
        frames.append((box, np.stack(planes)))
    assert at == len(raw)
    return {"nset": nset, "istart": istart, "nsavc": nsavc, "byte20": rest[0], "zeros": rest[1:], "delta": delta, "natom": natom}, frames


@pytest.mark.parametrize("with_box,skip_drude", [(True, False), (True, True), (False, False), (False, True)])
def test_the_reporter_writes_what_frame_of_says(with_box, skip_drude, tmp_path):
    s, _, _ = synth.nacl()
    x = s.positions + WSHIFT
    ctx = FrameStandIn(x, np.zeros(len(x)), s.resid, s.pair_drude, "mixed", BOX if with_box else None)
    path = tmp_path / "traj.dcd"
    rep = DCDReporter(str(path), 50, skip_drude=skip_drude)
    want = []
    for k in range(3):
        ctx.steps = 100 + 50 * k
        assert rep.due(ctx.steps) and not rep.due(ctx.steps + 1)
        ctx.posq[:, :3] += np.float32(0.11)                     # the molecules wander between frames
        rep.report(ctx)
        flags = (WRAP if with_box else 0) | (SKIP_DRUDE if skip_drude else 0)
        want.append(frame_of((ctx.posq, ctx.corr), ctx.labels, s.pair_drude, ctx.box, flags, 10.0, "mixed"))
        head, frames = parse_dcd(path.read_bytes(), with_box)   # the counters are current after every frame
        assert head["nset"] == k + 1 == len(frames) and head["byte20"] == ctx.steps
    rep.close()
    assert ctx.asked == [(with_box, skip_drude, 10.0, True)] * 3
    head, frames = parse_dcd(path.read_bytes(), with_box)
    natom = 2500 - (512 if skip_drude else 0)
    assert head == {"nset": 3, "istart": 100, "nsavc": 50, "byte20": 200, "zeros": (0,) * 5, "delta": np.float32(0.001), "natom": natom}
    lengths = [np.sqrt((BOX[k] ** 2).sum()) * 10.0 for k in range(3)]
    ang = lambda u, v: np.degrees(np.arccos(np.dot(u, v) / np.sqrt(np.dot(u, u) * np.dot(v, v))))   # noqa: E731
    for (cell, planes), w in zip(frames, want):
        assert planes.shape == (3, natom) and planes.tobytes() == np.ascontiguousarray(w.T).tobytes()       # bit for bit
        if with_box:
            np.testing.assert_allclose(cell, [lengths[0], ang(BOX[0], BOX[1]), lengths[1], ang(BOX[0], BOX[2]), ang(BOX[1], BOX[2]), lengths[2]],
                                       rtol=1e-14)
            assert 60 < min(cell[1], cell[3], cell[4]) and max(cell[1], cell[3], cell[4]) < 120
        else:
            assert cell is None
    if with_box:                                                # wrapped: frames differ from the plain ones
        assert not np.array_equal(want[0], frame_of((ctx.posq, ctx.corr), ctx.labels, s.pair_drude, None, flags & SKIP_DRUDE, 10.0, "mixed"))


def test_the_reporter_does_as_it_is_told():
    s, _, _ = synth.water_box(4)
    ctx = FrameStandIn(s.positions + WSHIFT, np.zeros(20), s.resid, s.pair_drude, "double", BOX)
    buf = io.BytesIO()
    rep = DCDReporter(buf, 10, enforcePeriodicBox=False)
    rep.report(ctx)
    assert ctx.asked == [(False, False, 10.0, True)]
    head, frames = parse_dcd(buf.getvalue(), True)              # the cell is written all the same
    assert head["natom"] == 20 and head["nset"] == 1 and head["delta"] == 0.0      # (no integrator, step 0: no step size to be had)
    assert frames[0][1].tobytes() == np.ascontiguousarray(frame_of((ctx.posq, None), ctx.labels, [], None, 0, 10.0, "double").T).tobytes()
    (la, lb, lc), (alpha, beta, gamma) = cell_lengths_and_angles(np.diag([1.0, 2.0, 3.0]))
    assert (la, lb, lc) == (10.0, 20.0, 30.0) and (alpha, beta, gamma) == (90.0, 90.0, 90.0)
