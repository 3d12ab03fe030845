"""The ``(mode, storage)`` argument pair of the models with opt-in 16-bit activation storage (ResNet18Wakeword, TCNWakeword)."""
import torch

from .. import _native as nat

_MODES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _storage(mode, storage):
    """(matrix mode, storage) as torch dtypes.  A 16-bit storage must be the matrix mode: an operand in HBM then already has the
    matrix cores' type."""
    m, s = _MODES.get(mode, mode), _MODES.get(storage, storage)
    nat.act_code(m)
    if s is torch.float32:
        return m, s
    if s not in (torch.bfloat16, torch.float16):
        raise ValueError(f"storage must be 'fp32', 'bf16' or 'fp16', got {storage!r}")
    if s is not m:
        raise ValueError(f"16-bit activation storage must equal the matrix mode: storage={storage!r} with mode={mode!r}")
    return m, s
