"""Colour grades: recolour and fade resident splats in place (include/gsplat/gs_abi.h "colour grades").

Free functions over a ``Renderer`` or a ``PipelinedRenderer`` (whose splats live with its first member: every slot is drained,
then that member is asked), like ``gsplat.neighbours`` and ``gsplat.clusters``.  Every other call either chooses splats or moves
them; these change what the chosen ones look like, on the device -- what would otherwise take export_splats (320 bytes per
splat), an edit of 48 SH floats per splat on the host and a re-upload that drops the frame, the shadows and every per-splat plane:

    r.select_sphere(c, 0.4); colours.brighten(r, 1.2); colours.saturate(r, 0.8)   # match one capture to another
    colours.tint(r, (1.05, 1.0, 0.9))                                             # warmer
    colours.levels(r, 0.03, 0.95)                                                 # black and white points
    colours.fade(r, 0.25)                                                         # a ghost of the selection

A grade is an affine map of the DISPLAYED colour, C' = diag(gain) Sat(saturation) ((C - black) / (white - black)) + offset.
Applied to the SH coefficients it holds in every view direction, exactly in real arithmetic wherever the renderer's final
max(0, .) is inactive before and after; the device applies exactly the f32 numbers of the GsGrade, with one rounding per operation,
so a host can restate it bit for bit.  fade multiplies the ODDS op / (1 - op) of the opacity (the logit gets log(gain) added), which
is about the opacity itself where it is small and never leaves (0, 1).  The calls are not frames and not uploads: the next frame
shows the grade.  The inverse grade is not a bit-exact undo: export the selection first if one is needed.
"""
import ctypes

from . import _abi
from ._abi import check
from .neighbours import _owner

_SEL = _abi.GS_SPLAT_SELECTED
MATRIX, OFFSET, OPACITY = _abi.GS_GRADE_MATRIX, _abi.GS_GRADE_OFFSET, _abi.GS_GRADE_OPACITY


def compose(gain=None, offset=None, saturation=1.0, black=0.0, white=1.0, opacity_gain=1.0):
    """gs_grade_compose (_abi.compose_grade): the GsGrade of the grade above.  Host mathematics in double, no GPU.  The flags name
    the parts that do something: the defaults compose a grade with flags == 0."""
    return _abi.compose_grade(gain, offset, saturation, black, white, opacity_gain)


def apply(r, grade, mask=_SEL, value=_SEL):
    """gs_grade_splats: applies a GsGrade in place to the resident splats with (s & mask) == value (default: the selection; (0, 0):
    every splat, also without GS_FLAG_SPLAT_STATE); returns how many those are.  Completes every frame in flight first."""
    o = _owner(r)
    matched = ctypes.c_uint64()
    check(o._L.gs_grade_splats(o._ctx, int(mask), int(value), ctypes.byref(grade), ctypes.byref(matched)))
    return int(matched.value)


# ---- the editor's verbs, all on the selection --------------------------------------------------------------------------------------
def brighten(r, factor):
    """Multiplies the displayed colour of the selection by `factor`; returns how many splats that is."""
    return apply(r, compose(gain=(factor, factor, factor)))


def tint(r, rgb):
    """Multiplies the displayed (r, g, b) of the selection by the three gains `rgb`."""
    return apply(r, compose(gain=rgb))


def saturate(r, saturation):
    """Moves the displayed colour of the selection towards (saturation < 1) or away from (> 1) its Rec. 709 luma; 0 is grey."""
    return apply(r, compose(saturation=saturation))


def levels(r, black, white):
    """Maps the displayed value `black` of the selection to 0 and `white` to 1."""
    return apply(r, compose(black=black, white=white))


def fade(r, opacity_gain):
    """Multiplies the odds of the selection's opacities by `opacity_gain` (> 0): about the opacity itself where it is small."""
    return apply(r, compose(opacity_gain=opacity_gain))
