"""Apodization plug-ins (class-name lookup namespace for ``ApodizationMethod.from_dict``).

``Uniform`` needs no geometry; ``MaxAngle`` and ``PiecewiseLinear`` get the element-normal-to-ray angle
from HIP kernel 1.  ``MediumCompensated`` (amplitudes through the attenuation of ``params``, HIP kernel 1a over one of the
three) is this package's extension.
"""
from __future__ import annotations

from . import apodmethod as _base
from . import maxangle as _maxangle
from . import mediumcompensated as _medcomp
from . import piecewiselinear as _pwl
from . import uniform as _uniform

ApodizationMethod = _base.ApodizationMethod
Uniform = _uniform.Uniform
MaxAngle = _maxangle.MaxAngle
PiecewiseLinear = _pwl.PiecewiseLinear
MediumCompensated = _medcomp.MediumCompensated

__all__ = ("ApodizationMethod", "Uniform", "MaxAngle", "PiecewiseLinear", "MediumCompensated")
