"""A Monte Carlo barostat for hosts without OpenMM: the stand-alone HipContext and particle-sharded runs.

Inside OpenMM leave it alone: the System's own MonteCarloBarostat acts there (the reference's example adds one,
example/nacl_tg.py:13-14, 56-57).  Here the trial move is the library's tgnh_scale_positions -- every molecule moved rigidly,
on the device, snapshot in the same launch -- and a rejected move is tgnh_restore_positions.  The library knows no potential
energy, and the move does not touch the library's periodic box: the caller hands in both, and after an accepted move sets the new
box itself (context.setPeriodicBoxVectors) where it wraps molecules or writes wrapped frames.
"""
import math

import numpy as np

from .synth import KB

AVOGADRO = 6.02214076e23


def _volume(box):
    return float(np.prod(box)) if box.ndim == 1 else abs(float(np.linalg.det(box)))


class MonteCarloBarostat:
    """MonteCarloBarostat(pressure_bar, temperature, frequency=25, seed=0).

    update(context, box, energy) -> (box, accepted) tries one volume move.  `context` is anything with flush() (optional),
    num_molecules(), scale_positions(scale, save=) and restore_positions() -- a HipContext, or a stand-in --; `box` the three
    edge lengths (nm) or the 3 x 3 box vectors; `energy` a callable context -> potential energy in kJ/mol (the caller's force
    call-out has it).  `frequency` is for the caller's loop (due(step_count)): update() itself always attempts a move.

    One update, as OpenMM's MonteCarloBarostat is recalled (OpenMM was not at hand to check against):
        E0 = energy(context);  dV = volumeScale 2 (u1 - 0.5);  s = ((V + dV) / V)^(1/3)
        context.scale_positions(s, save=True);  box' = s box;  E1 = energy(context)
        w = E1 - E0 + P dV - M kT ln(V' / V)       P = pressure_bar N_A 1e-25 kJ/mol/nm^3, M = context.num_molecules(), kT = KB T
        rejected iff w > 0 and u2 > exp(-w / kT):  context.restore_positions(), the old box is returned
        every 10 attempts: acceptance < 25 %: volumeScale /= 1.1;  > 75 %: volumeScale = min(1.1 volumeScale, 0.3 V)
    volumeScale starts at 0.01 V at the first update.  u1, u2 are drawn from numpy.random.default_rng(seed), both at every update,
    in this order.  Molecules scale about the origin and nothing is wrapped: this differs from OpenMM, which scales about the
    box's centre and keeps molecules in the box, only by whole box vectors.

    Before the move the context is flushed (a half kick still owed to the velocities belongs to the old positions' forces).
    After an accepted move the forces in the context's buffer are those of the old positions: recomputing them is left to the
    caller's next force call, before the next step.  The harness' tether sites (HipContext.set_sites) are NOT scaled.
    """

    def __init__(self, pressure_bar, temperature, frequency=25, seed=0):
        self.pressure = float(pressure_bar) * AVOGADRO * 1e-25      # kJ/mol/nm^3
        self.kT = KB * float(temperature)
        self.frequency = int(frequency)
        self.rng = np.random.default_rng(seed)
        self.volume_scale = None
        self.attempted = self.accepted = 0                           # since the last adaptation
        self.total_attempted = self.total_accepted = 0

    def due(self, step_count):
        return self.frequency > 0 and step_count % self.frequency == 0

    def update(self, context, box, energy):
        box = np.asarray(box, np.float64)
        volume = _volume(box)
        if self.volume_scale is None:
            self.volume_scale = 0.01 * volume
        if hasattr(context, "flush"):
            context.flush()
        u1, u2 = self.rng.random(), self.rng.random()
        e0 = float(energy(context))
        dv = self.volume_scale * 2.0 * (u1 - 0.5)
        new_volume = volume + dv
        s = (new_volume / volume) ** (1.0 / 3.0)
        context.scale_positions(s, save=True)
        e1 = float(energy(context))
        w = e1 - e0 + self.pressure * dv - context.num_molecules() * self.kT * math.log(new_volume / volume)
        accepted = not (w > 0.0 and u2 > math.exp(-w / self.kT))
        if accepted:
            box = box * s
            volume = new_volume
        else:
            context.restore_positions()
        self.attempted += 1
        self.accepted += int(accepted)
        self.total_attempted += 1
        self.total_accepted += int(accepted)
        if self.attempted >= 10:
            if self.accepted < 0.25 * self.attempted:
                self.volume_scale /= 1.1
            elif self.accepted > 0.75 * self.attempted:
                self.volume_scale = min(self.volume_scale * 1.1, volume * 0.3)
            self.attempted = self.accepted = 0
        return box, accepted
