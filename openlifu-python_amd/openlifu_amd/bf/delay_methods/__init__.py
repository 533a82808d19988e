"""Delay-method plug-ins.

Namespace used for class-name lookup: ``DelayMethod.from_dict({"class": "Direct", ...})`` resolves
``"Direct"`` here, exactly like the reference's package of the same name.  ``StraightRay`` (aberration
correction through the ``params`` medium) is this package's extension.
"""
from __future__ import annotations

from . import delaymethod as _base
from . import direct as _direct
from . import straightray as _straightray

DelayMethod = _base.DelayMethod
Direct = _direct.Direct
StraightRay = _straightray.StraightRay

__all__ = ("DelayMethod", "Direct", "StraightRay")
