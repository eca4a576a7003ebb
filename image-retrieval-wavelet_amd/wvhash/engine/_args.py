"""The argument gate of engine/hamming.py and engine/hamming_host.py: every tensor whose pointer goes to the C ABI
(include/wvhash.h) passes gate() first.  The entry points take raw pointers and read Q, N, words and k rows of the declared
type behind them; a strided view or a wider dtype would be read in bounds and give a wrong ranking or metric without any
error, a narrower dtype, fewer rows or a tensor of another device would be read out of bounds.  The rules are decided
here, not per wrapper.  Pure Python on tensor metadata: no value is read (.item(), .any()), nothing synchronises with the
device -- the gate sits in the per-step path."""
import torch

ROWS = "rows"            # input read as plain contiguous rows: any stride or storage offset is accepted, copied when not contiguous
PITCH = "pitch"          # 2-D input whose entry point takes a row pitch: stride(1) == 1 and stride(0) >= shape[1] stay as they are
WRITTEN = "written"      # buffer the entry point writes: never copied -- it is right as it stands or refused
INDEX = "index"          # declared dtype of a ranked index list: int32; int64 (what get_knn hands out, idx.long()) is converted


def anchor(t, what, name, device_type):
    """The device every tensor argument of wrapper `what` must live on: that of its first tensor argument `t` (named `name`),
    which must be of the module's kind ('cuda' for engine/hamming.py, 'cpu' for engine/hamming_host.py)."""
    if not torch.is_tensor(t):
        raise ValueError(f"{what}: {name}: expected a tensor, got {type(t).__name__}")
    if t.device.type != device_type:
        raise ValueError(f"{what}: {name}: expected a tensor on a {device_type} device, got one on {t.device}")
    return t.device


def same_device(obj, what, name, device):
    """A prepared object (PreparedDB, PreparedLabels: anything with .packed) lives on the anchor device."""
    if obj.packed.device != device:
        raise ValueError(f"{what}: {name}: lives on {obj.packed.device}, the other arguments on {device}")
    return obj


def gate(t, what, name, dtype, device, shape, kind=ROWS):
    """-> a tensor that is safe to take a pointer from, or ValueError naming the wrapper `what` and the argument `name`.
    dtype: the declared torch dtype, or INDEX; device: the anchor device (anchor()); shape: one entry per dimension, None
    where any extent goes; kind: ROWS, PITCH or WRITTEN.  A canonical tensor comes back as it is (same data_ptr())."""
    if not torch.is_tensor(t):
        raise ValueError(f"{what}: {name}: expected a tensor, got {type(t).__name__}")
    if t.device != device:
        raise ValueError(f"{what}: {name}: lives on {t.device}, expected {device}")
    if t.dim() != len(shape) or any(want is not None and have != want for have, want in zip(t.shape, shape)):
        wanted = "[" + ", ".join("*" if s is None else str(s) for s in shape) + "]"
        raise ValueError(f"{what}: {name}: expected shape {wanted}, got {list(t.shape)}")
    declared = torch.int32 if dtype is INDEX else dtype
    if t.dtype != declared:
        if not (dtype is INDEX and t.dtype == torch.int64 and kind != WRITTEN):
            raise ValueError(f"{what}: {name}: expected dtype {declared}, got {t.dtype}")
        t = t.to(torch.int32)
    if kind == WRITTEN:
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name}: a buffer that is written must be contiguous (strides {tuple(t.stride())})")
        return t
    if kind == PITCH and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t
    return t.contiguous()
