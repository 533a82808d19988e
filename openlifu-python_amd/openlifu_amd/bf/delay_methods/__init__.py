"""Delay-method plug-ins.

Namespace used for class-name lookup: ``DelayMethod.from_dict({"class": "Direct", ...})`` resolves
``"Direct"`` here, exactly like the reference's package of the same name.  ``StraightRay`` (aberration
correction through the ``params`` medium) and ``TimeReversal`` (delays from one full-wave
run per focus, refraction and reflection included) are this package's extensions, as is ``Eikonal`` (refracted
first-arrival travel times, two eikonal solves per focus: between the two in cost).
"""
from __future__ import annotations

from . import delaymethod as _base
from . import direct as _direct
from . import eikonal as _eikonal
from . import straightray as _straightray
from . import timereversal as _timereversal

DelayMethod = _base.DelayMethod
Direct = _direct.Direct
StraightRay = _straightray.StraightRay
TimeReversal = _timereversal.TimeReversal
Eikonal = _eikonal.Eikonal

__all__ = ("DelayMethod", "Direct", "StraightRay", "TimeReversal", "Eikonal")
