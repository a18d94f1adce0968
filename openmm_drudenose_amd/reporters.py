"""Trajectory output for hosts without OpenMM: DCDFile writes CHARMM DCD, DCDReporter feeds it from a context.

Inside OpenMM leave it alone: the application layer's DCDReporter acts there (the reference's example adds one,
example/nacl_tg.py).  Here a frame is the library's tgnh_write_frame -- fp32 coordinates in Angstrom, three planes, molecules
wrapped into the periodic cell on the way, formed on the device -- so 12 bytes per atom cross to the host instead of the fp64
positions, and nothing of the trajectory is touched.

The format is little-endian CHARMM DCD as OpenMM's DCDFile writes it, RECALLED FROM MEMORY: mdtraj, MDAnalysis and OpenMM were not
at hand to read a file back with, so tests/test_wrap_frames.py parses it by this layout and nothing else vouches for it.

    header    int32 84, 'CORD', 9 int32 (NSET = 0, ISTART = first step, NSAVC = interval, six zeros), float32 DELTA = step size in
              ps, 10 int32 (1 where frames carry a cell, eight zeros, 24), int32 84
    title     int32 164, int32 2, two 80-byte lines, int32 164
    atoms     int32 4, int32 NATOM, int32 4
    per frame with a cell: int32 48, six float64 (|a|, gamma, |b|, beta, alpha, |c|: lengths in Angstrom, angles in degrees), int32 48;
              then for each of x, y, z: int32 4 NATOM, NATOM float32 in Angstrom, int32 4 NATOM
    after every frame NSET is rewritten at byte 8 and the last step's number at byte 20
"""
import math
import struct

import numpy as np


def cell_lengths_and_angles(box):
    """box vectors [3, 3] in nm -> (|a|, |b|, |c|) in Angstrom and (alpha, beta, gamma) in degrees: alpha between b and c, beta
    between a and c, gamma between a and b"""
    a, b, c = (np.asarray(v, np.float64) for v in box)
    la, lb, lc = (math.sqrt(float(np.dot(v, v))) for v in (a, b, c))
    alpha = math.degrees(math.acos(float(np.dot(b, c)) / (lb * lc)))
    beta = math.degrees(math.acos(float(np.dot(a, c)) / (la * lc)))
    gamma = math.degrees(math.acos(float(np.dot(a, b)) / (la * lb)))
    return (10.0 * la, 10.0 * lb, 10.0 * lc), (alpha, beta, gamma)


class DCDFile:
    """DCDFile(file, natom, dt, first_step=0, interval=1, cell=False): the header is written at once; write_frame(planes, box,
    step) appends a frame and brings the header's counters up to date.  `file` is a path or a binary file open for writing that
    can seek."""

    def __init__(self, file, natom, dt, first_step=0, interval=1, cell=False):
        self._own = isinstance(file, (str, bytes)) or hasattr(file, "__fspath__")
        self._f = open(file, "wb") if self._own else file
        self.natom, self.cell, self.frames = int(natom), bool(cell), 0
        title = [b"Created by openmm_drudenose_amd", b"coordinates in Angstrom; molecules wrapped where a cell is given"]
        head = struct.pack("<i4s9if10ii", 84, b"CORD", 0, int(first_step), int(interval), 0, 0, 0, 0, 0, 0, float(dt),
                           int(self.cell), 0, 0, 0, 0, 0, 0, 0, 0, 24, 84)
        head += struct.pack("<ii", 164, 2) + b"".join(line.ljust(80)[:80] for line in title) + struct.pack("<i", 164)
        head += struct.pack("<iii", 4, self.natom, 4)
        self._start = self._f.tell()
        self._f.write(head)

    def write_frame(self, planes, box=None, step=0):
        """planes: float32 [3, natom], Angstrom; box: the three box vectors in nm where the file carries a cell"""
        planes = np.ascontiguousarray(planes, "<f4")
        if planes.shape != (3, self.natom):
            raise ValueError(f"DCDFile: a frame is three planes of {self.natom} float32, got {planes.shape}")
        if self.cell != (box is not None):
            raise ValueError("DCDFile: every frame of a file carries a cell, or none does")
        f = self._f
        if self.cell:
            (la, lb, lc), (alpha, beta, gamma) = cell_lengths_and_angles(box)
            f.write(struct.pack("<i6di", 48, la, gamma, lb, beta, alpha, lc, 48))
        mark = struct.pack("<i", 4 * self.natom)
        for k in range(3):
            f.write(mark)
            f.write(planes[k].tobytes())
            f.write(mark)
        self.frames += 1
        end = f.tell()
        f.seek(self._start + 8)
        f.write(struct.pack("<i", self.frames))
        f.seek(self._start + 20)
        f.write(struct.pack("<i", int(step)))
        f.seek(end)
        f.flush()

    def close(self):
        if self._own and not self._f.closed:
            self._f.close()


class DCDReporter:
    """DCDReporter(file, reportInterval, enforcePeriodicBox=None, skip_drude=False): report(context) appends the context's
    positions as one frame; the caller's loop decides when (due(step_count): every reportInterval steps).

    `context` is anything with frame(wrap=, skip_drude=, unit=, planes=), frame_count(skip_drude), getPeriodicBoxVectors() and
    time() -> (ps, step count) -- a HipContext, or a stand-in.  enforcePeriodicBox=None wraps whole molecules into the cell
    whenever the context has a box (and writes the cell with every frame); True / False say so outright.  skip_drude=True leaves
    the Drude particles out of the file.  The file is created at the first report: ISTART is that report's step count."""

    def __init__(self, file, reportInterval, enforcePeriodicBox=None, skip_drude=False):
        self._file, self._out = file, None
        self.reportInterval = int(reportInterval)
        self.enforcePeriodicBox, self.skip_drude = enforcePeriodicBox, bool(skip_drude)

    def due(self, step_count):
        return self.reportInterval > 0 and step_count % self.reportInterval == 0

    def report(self, context):
        t, step = context.time()
        box = context.getPeriodicBoxVectors()
        wrap = (box is not None) if self.enforcePeriodicBox is None else bool(self.enforcePeriodicBox)
        if self._out is None:
            integrator = getattr(context, "integrator", None)
            dt = integrator.getStepSize() if integrator is not None else (t / step if step else 0.0)
            self._out = DCDFile(self._file, context.frame_count(self.skip_drude), dt, step, self.reportInterval, box is not None)
        planes = context.frame(wrap=wrap, skip_drude=self.skip_drude, unit=10.0, planes=True)
        if hasattr(planes, "cpu"):
            planes = planes.cpu().numpy()                   # (the one copy to the host: 12 bytes per atom)
        self._out.write_frame(planes, box, step)

    def close(self):
        if self._out is not None:
            self._out.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
