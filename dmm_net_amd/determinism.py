"""Deterministic mode: bit-identical training steps for the same inputs and seeds, run after run, graph replay and eager alike.

Off by default.  ``None`` (the default setting) follows torch: the mode is on while
``torch.are_deterministic_algorithms_enabled()`` or ``torch.backends.cudnn.deterministic`` is -- so a training script that sets
``torch.backends.cudnn.deterministic = True`` (the reference's ``train.py:46``) gets it without edits.  An explicit
``set_deterministic(True / False)`` wins over torch's flags.

In the mode the reductions that add float partials in arrival order (BatchNorm statistics and backward sums, bias gradients,
the mask-mix backward's dRb, the ROIAlign+mean backward) take their ``_det`` entries (include/dmm_match.h): fixed-order folds
of per-workgroup slabs and a gather, no float atomics.  The library calls run under ``cudnn.deterministic``; DESIGN.md
"Deterministic mode" records what that needed and what it costs.

``set_deterministic_conv("own")`` takes the mode's 3x3 convolutions (forward and data gradient) off MIOpen -- which answers
``cudnn.deterministic`` with its naive reference kernel on gfx950 -- and onto ``dmm_conv3x3_bf16``; ``"library"`` (the
default) leaves every route as it is.  ``"own_all"`` is ``"own"`` plus the narrow 3x3 convolutions (stride 1, widths that
are multiples of 32 but not of 64: the 32-channel level-2 heads), which ``"own"`` runs as unfold + GEMM: forward and data
gradient on ``dmm_conv3x3_narrow_bf16``, the weight gradient on ``dmm_wgrad3x3_narrow_bf16``.  ``"own_stem"`` is ``"own_all"``
plus the 7x7 / stride 2 stem (3 -> 64), the last convolution on unfold + GEMM: forward on ``dmm_conv7x7s2_stem_bf16``, weight
gradient (fp32 from the kernel) on ``dmm_wgrad7x7s2_stem_bf16`` -- a deterministic ResNet step then holds no library
convolution and no unfold.  The setting has no effect while the mode is off."""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

_SETTING: Optional[bool] = None
_CONV: str = "library"


def set_deterministic(mode: Optional[bool]) -> None:
    """True / False: force the mode on / off; None: follow torch's flags (the default)."""
    global _SETTING
    if mode is not None and not isinstance(mode, bool):
        raise TypeError("set_deterministic takes True, False or None")
    _SETTING = mode


def get_deterministic_setting() -> Optional[bool]:
    """The explicit setting (None = following torch)."""
    return _SETTING


def set_deterministic_conv(which: str) -> None:
    """Who computes the 3x3 convolutions of a deterministic step: ``"library"`` (MIOpen under cudnn.deterministic, the default),
    ``"own"`` (``dmm_conv3x3_bf16`` for every 3x3 / padding 1 convolution with widths that are multiples of 64),
    ``"own_all"`` (``"own"``, and ``dmm_conv3x3_narrow_bf16`` / ``dmm_wgrad3x3_narrow_bf16`` for the stride-1 ones whose widths
    are multiples of 32 only) or ``"own_stem"`` (``"own_all"``, and ``dmm_conv7x7s2_stem_bf16`` / ``dmm_wgrad7x7s2_stem_bf16``
    for the 7x7 / stride 2 / padding 3 stem, 3 -> 64)."""
    global _CONV
    if not isinstance(which, str) or which not in ("library", "own", "own_all", "own_stem"):
        raise ValueError('set_deterministic_conv takes "library", "own", "own_all" or "own_stem"')
    _CONV = which


def get_deterministic_conv() -> str:
    return _CONV


def is_deterministic() -> bool:
    """The mode as it resolves now: one cheap check per call of the dispatching ops."""
    if _SETTING is not None:
        return _SETTING
    return bool(torch.backends.cudnn.deterministic) or torch.are_deterministic_algorithms_enabled()


@contextlib.contextmanager
def deterministic(mode: Optional[bool] = True):
    """``with dmm_net_amd.deterministic(): ...`` -- the mode for a block; the previous setting is restored on exit."""
    old = _SETTING
    set_deterministic(mode)
    try:
        yield
    finally:
        set_deterministic(old)


@contextlib.contextmanager
def library_flags(on: bool):
    """cudnn.deterministic for the library calls of a deterministic step (MIOpen's solver picks are made under it); a no-op
    when the mode is off, so the default path's settings are untouched."""
    if not on or torch.backends.cudnn.deterministic:
        yield
        return
    with torch.backends.cudnn.flags(enabled=torch.backends.cudnn.enabled, benchmark=torch.backends.cudnn.benchmark,
                                    deterministic=True, allow_tf32=torch.backends.cudnn.allow_tf32):
        yield
