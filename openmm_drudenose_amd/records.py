"""What the feature calls hand back and take: the read-only result records (`DrudeStatistics`, `Momentum`, `MinimizeState`) and
the minimiser's descriptor."""
import numpy as np

from . import _lib
from ._abi import Record, TgnhError


class DrudeStatistics(Record):
    """What HipContext.drude_statistics returns (read-only): pairs, over (pairs beyond `threshold`), max_distance and rms_distance
    (nm), worst_particle (slot of the Drude particle of the longest pair, -1: no pair), induced_dipole (e nm, 3 values), hist
    (int64, 33 values: 32 bins of width hist_max / 32, then the pairs at or beyond hist_max; zeros when hist_max == 0) and
    hist_edges (the 33 edges of the 32 bins; None when hist_max == 0)."""
    __slots__ = ("pairs", "over", "max_distance", "rms_distance", "worst_particle", "induced_dipole", "hist", "hist_edges",
                 "sum_d2", "threshold", "hist_max", "raw")

    def __init__(self, st, threshold, hist_max):
        self._fill(st, pairs=int(st.pairs), over=int(st.over), worst_particle=int(st.worst_particle),
                   max_distance=float(st.max_distance), sum_d2=float(st.sum_d2),
                   rms_distance=float(np.sqrt(st.sum_d2 / st.pairs)) if st.pairs else 0.0, threshold=threshold, hist_max=hist_max,
                   induced_dipole=np.array(st.dipole[:], np.float64), hist=np.array(st.hist[:], np.int64),
                   hist_edges=np.linspace(0.0, hist_max, _lib.DRUDE_HIST_BINS + 1) if hist_max > 0 else None)

    def __repr__(self):
        return (f"DrudeStatistics(pairs={self.pairs}, over={self.over}, max_distance={self.max_distance:.6g}, "
                f"rms_distance={self.rms_distance:.6g}, worst_particle={self.worst_particle}, induced_dipole={self.induced_dipole.tolist()})")


class Momentum(Record):
    """What HipContext.momentum returns (read-only): mass (amu) and momentum (amu nm/ps, 3 values) of the context's massive slots,
    massive (their number) and velocity = momentum / mass, the centre-of-mass velocity (zeros when there is no mass)."""
    __slots__ = ("mass", "momentum", "massive", "velocity", "raw")

    def __init__(self, st):
        p = np.array(st.momentum[:], np.float64)
        self._fill(st, mass=float(st.mass), massive=int(st.massive), momentum=p, velocity=p / st.mass if st.mass != 0 else np.zeros(3))

    def __repr__(self):
        return f"Momentum(mass={self.mass:.6g}, momentum={self.momentum.tolist()}, massive={self.massive}, velocity={self.velocity.tolist()})"


class MinimizeState(Record):
    """What HipContext.minimizeEnergy and minimize_state return (read-only): tgnh_minimize_state as the last decision left it --
    iterations (updates made), uphill (resets), since_uphill, moving (this context's moving slots), converged (0 running, 1 the
    rms force is <= tolerance, -1 a sum was not finite), dt, alpha, power (f.v), ff, vv and rms_force (kJ/mol/nm)."""
    __slots__ = ("iterations", "uphill", "since_uphill", "moving", "converged", "dt", "alpha", "power", "ff", "vv", "rms_force", "raw")

    def __init__(self, st):
        self._fill(st, **{k: int(getattr(st, k)) for k in ("iterations", "uphill", "since_uphill", "moving", "converged")},
                   **{k: float(getattr(st, k)) for k in ("dt", "alpha", "power", "ff", "vv", "rms_force")})

    def __repr__(self):
        return (f"MinimizeState(iterations={self.iterations}, converged={self.converged}, rms_force={self.rms_force:.6g}, "
                f"uphill={self.uphill}, dt={self.dt:.6g}, alpha={self.alpha:.6g}, moving={self.moving})")


FIRE_DEFAULTS = dict(dt_start=1e-4, dt_max=1e-3, max_step=0.01, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99, n_min=5)


def minimize_desc(n, tolerance=10.0, drude_only=False, moving=None, **fire):
    """-> (tgnh_minimize_desc, the mask array it points to or None: keep it alive for the call).  **fire: FIRE_DEFAULTS' names."""
    unknown = set(fire) - set(FIRE_DEFAULTS)
    if unknown:
        raise TgnhError(_lib.ERR_ARG, f"minimize: unknown FIRE parameter(s) {sorted(unknown)}")
    par = dict(FIRE_DEFAULTS, **fire)
    d = _lib.TgnhMinimizeDesc()
    d.tolerance = float(tolerance)
    for k, v in par.items():
        setattr(d, k, int(v) if k == "n_min" else float(v))
    d.flags = _lib.MIN_DRUDE_ONLY if drude_only else 0
    mask = None
    if moving is not None:
        mask = np.ascontiguousarray(np.asarray(moving) != 0, np.uint8)
        if mask.shape != (n,):
            raise TgnhError(_lib.ERR_ARG, "minimize: one mask entry per particle slot")
        d.moving = mask.ctypes.data
    return d, mask
