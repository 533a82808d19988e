"""Simulation grid + the ``run_simulation`` seam (HIP kernel 2 instead of k-Wave) + the thermal model (HIP kernel 3) + the opt-in
full-wave field model (HIP kernel 5)."""
from __future__ import annotations

from . import field
from . import fullwave
from . import sim_setup as _sim_setup
from . import thermal

run_simulation = field.run_simulation
SimSetup = _sim_setup.SimSetup
run_thermal_simulation = thermal.run_thermal_simulation
run_fullwave_simulation = fullwave.run_fullwave_simulation
run_fullwave_steady_state = fullwave.run_fullwave_steady_state

__all__ = ("SimSetup", "run_simulation", "run_thermal_simulation", "run_fullwave_simulation", "run_fullwave_steady_state", "field", "thermal", "fullwave")
