"""The import point of the Python surface over the HIP C ABI: re-exports only.  `DrudeTGNHIntegrator` mirrors the reference's SWIG
wrapper (python/drudetgnhplugin.i:60-92 of scychon/openmm_drudeNose); `HipContext` stands where OpenMM's Context + HIP platform
would.  Which module holds what: DESIGN.md, "The Python surface"."""
from ._lib import (MODE_DUALNH, MODE_TGNH, PREC_SINGLE, PREC_MIXED, PREC_DOUBLE,  # noqa: F401
                   FLAG_DEFER_SCALE, FLAG_RESIDENT_STEP, FLAG_WAVE_TILES, FLAG_TRUST_STATE_CHANGED, FLAG_GATHER)
from .synth import KB  # noqa: F401
from ._abi import TgnhError, _check  # noqa: F401
from .integrator import DrudeTGNHIntegrator  # noqa: F401
from .handle import MAX_DIRECT_CONSTRAINTS, HostTopology, create_handle, split_clusters  # noqa: F401
from .records import FIRE_DEFAULTS, DrudeStatistics, MinimizeState, Momentum, minimize_desc  # noqa: F401
from .context import HipContext  # noqa: F401
