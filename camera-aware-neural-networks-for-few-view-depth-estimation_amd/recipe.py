"""The declared training recipe's learning-rate schedule (cad_lr_at, host only: no torch, no device).

The reference's Trainer (src/training/trainer.h:262-308) sets the warmup rate directly for epochs below
lr_warmup_epochs and calls scheduler.step() after every later epoch; over StepLR / CosineAnnealingLR(T_max =
num_epochs - warmup, eta_min = lr_min) that loop has the closed forms cad_lr_at evaluates.
"""
from __future__ import annotations

import ctypes as C

from . import _abi

SCHEDULERS = ("none", "step", "cosine")


def lr_at(epoch, num_epochs, lr, scheduler="none", step_size=30, gamma=0.1, warmup_epochs=0, lr_min=0.0) -> float:
    """Learning rate of 0-based `epoch` out of `num_epochs` (the float32 the trainers set).  ValueError naming
    the scheduler for "plateau" and unknown names."""
    lib = _abi.load()
    name = "none" if scheduler is None else str(scheduler)
    o = _abi.LrOpts(float(lr), name.encode(), int(step_size), float(gamma), int(warmup_epochs), float(lr_min))
    out = C.c_float()
    if lib.cad_lr_at(C.byref(o), int(epoch), int(num_epochs), C.byref(out)) != 0:
        raise ValueError(lib.cad_last_error().decode(errors="replace"))
    return float(out.value)
