"""Sizing on the device: the workers record the geometry, the GPU touches the pixels.

With ``build_transform(cfg, defer=True, sizing="device")`` the geometry steps of a pipeline (``Resize``, ``CenterCrop``,
``RandomResizedCrop``, ``RandomHorizontalFlip`` and the wavelet plugin's BICUBIC ``fix_size``) receive a ``LazyImage``
instead of a PIL image: it answers ``.size`` / ``.resize`` / ``.crop`` / ``.transpose`` like one, but only logs the calls.
The plugin at the end of the pipeline turns the log into ``wv_size_stage`` records (include/wvhash.h) and returns a
``RawItem``: the decoded image untouched plus its records.  ``raw_collate`` packs the items of a batch into a ``RawBatch``
(one byte buffer, one descriptor tensor), ``functional.size_images`` runs one ``wv_image_size`` launch per stage index on
the GPU and returns ``uint8 [B, H, W, 3]`` -- bit-identical to what Pillow makes of the same calls.

How calls become stages (one stage = crop -> resample -> window / zero pad -> mirror):
* a crop before the stage's resample narrows its crop rectangle, a crop after it moves its window (which may hang over the
  resampled image: zero pad, like ``Image.crop`` and torchvision's ``CenterCrop`` of a too small image);
* a mirror toggles the stage's flag (a crop after a mirror is the mirrored crop of the window); a crop that hangs over an
  earlier crop's window opens a new stage (its zero pad is relative to that window, not to the image);
* a resample after a resample, after a mirror or after a padded window opens a new stage -- resampling and mirroring do not
  commute exactly, the ``(int)(x + 0.5)`` bounds of the resampler are not symmetric;
* a call Pillow answers with an unchanged copy (``resize`` to the size the image has) records nothing.
An image outside the kernel's limits (``wv_image_size_check`` answers WV_ENOTSUP), or one that is not 8-bit RGB, is sized
with PIL in the worker by replaying the log, and carries an empty stage list.

Colour operations (``ColorJitter``: brightness, contrast, saturation; ``wv_colour_ops`` records, ``wv_colour_jitter``) are not
geometry but ride on it: an operation attaches to the stage that is open when it is recorded (an identity stage if there is
none) and runs, in place, on what that stage wrote -- its whole window, zero pad included, as PIL would see it.
* a later mirror only toggles the flag: pointwise operations and a mean over the whole image commute with it;
* a later crop or resample opens a new stage: the contrast mean belongs to the image as it was;
* a stage holds one chain, each kind at most once.  A second operation of a kind on one stage, or a hue operation (which
  the kernel does not implement), sends the image down the PIL fallback above.
"""
import ctypes
import math
from collections.abc import Mapping

import numpy as np
import torch
from PIL import Image, ImageEnhance

from .. import _lib


class _Table(object):
    """One descriptor table of the C ABI: the numpy dtype of a record, its 32-bit words, the name of its ``*_check`` symbol."""

    def __init__(self, dtype, struct, check_name):
        self.dtype, self.words, self.check_name = np.dtype(dtype), ctypes.sizeof(struct) // 4, check_name
        assert self.dtype.itemsize == ctypes.sizeof(struct)

    def check(self, rec):
        """The table's check on host records -> return code (0, WV_EINVAL or WV_ENOTSUP); the message is wv_last_error()."""
        rec = np.ascontiguousarray(rec)
        return getattr(_lib.load(), self.check_name)(ctypes.c_void_p(rec.ctypes.data), len(rec))

    def require(self, rec):
        """The same check, raising: the descriptors pass on the host copy, the device entry points cannot read them."""
        _lib.check(self.check(rec), self.check_name)

    def tensor(self, chunks):
        """Record arrays -> one int32 [records, words] tensor (bit patterns)."""
        return torch.from_numpy(np.concatenate(chunks).view(np.int32).reshape(-1, self.words).copy())

    def address(self, tensor, first):
        """Where record `first` of such a tensor lies."""
        return ctypes.c_void_p(tensor.data_ptr() + first * self.words * 4)


STAGES = _Table([("src_offset", "<i8"), ("dst_offset", "<i8")] + [(n, "<i4") for n, _ in _lib.SizeStage._fields_[2:]],
                _lib.SizeStage, "wv_image_size_check")                        # wv_size_stage: 80 bytes
COLOURS = _Table([("offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("row_bytes", "<i4"), ("n_ops", "<i4"), ("kind", "<i4", (3,)),
                  ("factor", "<f4", (3,))], _lib.ColourOps, "wv_colour_jitter_check")   # wv_colour_ops: 48 bytes
STAGE_DTYPE, STAGE_WORDS, check_records = STAGES.dtype, STAGES.words, STAGES.check
COLOUR_DTYPE, COLOUR_WORDS, check_colour_records = COLOURS.dtype, COLOURS.words, COLOURS.check
COLOUR_KINDS = {"brightness": _lib.WV_COLOUR_BRIGHTNESS, "contrast": _lib.WV_COLOUR_CONTRAST,
                "saturation": _lib.WV_COLOUR_SATURATION}
_ENHANCERS = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}
_ALIGN = 16
_FILTERS = {int(Image.BILINEAR): _lib.WV_RESAMPLE_BILINEAR, int(Image.BICUBIC): _lib.WV_RESAMPLE_BICUBIC}


def _align(n):
    return (n + _ALIGN - 1) // _ALIGN * _ALIGN


def ksize(in_len, out_len, filt):
    """Taps of a coefficient row of one axis: csrc/image_size.hpp's axis_ksize, same double arithmetic."""
    if in_len == out_len:
        return 1
    return min(int(math.ceil((1.0 if filt == _lib.WV_RESAMPLE_BILINEAR else 2.0) * max(in_len / out_len, 1.0))) * 2 + 1, in_len)


def pil_colour(img, kind, factor):
    """One colour operation on a PIL image, as torchvision applies it to PIL input: ImageEnhance for brightness, contrast and
    saturation; for hue ``convert("HSV")``, ``int(factor * 255) & 0xFF`` added to H modulo 256, merged and converted back
    (images without colour -- modes L, 1, I, F -- are returned as they are)."""
    if kind in _ENHANCERS:
        return _ENHANCERS[kind](img).enhance(factor)
    if kind != "hue":
        raise ValueError(f"unknown colour operation {kind!r}")
    if not -0.5 <= factor <= 0.5:
        raise ValueError(f"hue factor {factor} is not in [-0.5, 0.5]")
    mode = img.mode
    if mode in ("L", "1", "I", "F"):
        return img
    h, s, v = img.convert("HSV").split()
    h = h.point([(i + (int(factor * 255) & 0xFF)) & 0xFF for i in range(256)])
    return Image.merge("HSV", (h, s, v)).convert(mode)


class NotRecordable(ValueError):
    """The call log describes something the stages cannot express (to_item sizes such an image with PIL)."""


def _fresh_stage(w, h):
    """A stage that shows a w x h image as it is."""
    return {"src_w": w, "src_h": h, "crop": [0, 0, w, h], "res": None, "win": [0, 0, w, h], "flip": 0,
            "filter": _lib.WV_RESAMPLE_BILINEAR, "colour": []}


def _shown(st):
    """(w, h) of the image the stage's window looks at: the resampled one, the crop where nothing is resampled."""
    rw, rh = st["res"] if st["res"] is not None else st["crop"][2:]
    return rw, rh


def stages_from_ops(width, height, ops):
    """The call log of a LazyImage -> list of stage dicts (sizes only, offsets and row pitches are the packer's).  A stage's
    "colour" is its chain [(kind name, factor), ...] in running order."""
    stages, cur = [], None
    w, h = width, height

    for op in ops:
        if op[0] == "resize":
            (nw, nh), filt = op[1], op[2]
            if (nw, nh) == (w, h):
                continue                                    # Pillow returns a copy: nothing is resampled
            if cur is None:
                cur = _fresh_stage(w, h)
            rw, rh = _shown(cur)
            x, y, ww, wh = cur["win"]
            padded = x < 0 or y < 0 or x + ww > rw or y + wh > rh
            if cur["res"] is not None or cur["flip"] or padded or cur["colour"]:
                stages.append(cur)
                cur = _fresh_stage(w, h)
                x, y, ww, wh = cur["win"]
            cx, cy = cur["crop"][:2]
            cur["crop"] = [cx + x, cy + y, ww, wh]          # the window of an unresampled stage is a crop
            cur["res"], cur["filter"], cur["win"] = (nw, nh), filt, [0, 0, nw, nh]
            w, h = nw, nh
        elif op[0] == "crop":
            x, y, cw, ch = op[1]
            if cur is None:
                cur = _fresh_stage(w, h)
            wx, wy, ww, wh = cur["win"]
            if cur["colour"]:
                stages.append(cur)                          # the contrast mean belongs to the image before the crop
                cur = _fresh_stage(w, h)
            elif (x < 0 or y < 0 or x + cw > ww or y + ch > wh) and [wx, wy, ww, wh] != [0, 0, *_shown(cur)]:
                stages.append(cur)                          # the zero pad is relative to the window, not to the image
                cur = _fresh_stage(w, h)
            if cur["flip"]:
                x = cur["win"][2] - x - cw
            cur["win"] = [cur["win"][0] + x, cur["win"][1] + y, cw, ch]
            w, h = cw, ch
        elif op[0] == "mirror":
            if cur is None:
                cur = _fresh_stage(w, h)
            cur["flip"] ^= 1
        elif op[0] == "colour":
            kind, factor = op[1], op[2]
            if cur is None:
                cur = _fresh_stage(w, h)
            if kind not in COLOUR_KINDS:
                raise NotRecordable(f"colour operation {kind!r} is not one of the kernel's")
            if any(k == kind for k, _ in cur["colour"]):
                raise NotRecordable(f"a second {kind} operation on one stage")
            cur["colour"].append((kind, float(factor)))
        else:
            raise ValueError(f"unknown sizing op {op[0]!r}")
    if cur is not None:
        stages.append(cur)
    return stages


def _records(stages):
    rec = np.zeros(len(stages), dtype=STAGE_DTYPE)
    for r, st in zip(rec, stages):
        rw, rh = _shown(st)
        r["src_h"], r["src_w"], r["src_row_bytes"] = st["src_h"], st["src_w"], 3 * st["src_w"]
        r["crop_x"], r["crop_y"], r["crop_w"], r["crop_h"] = st["crop"]
        r["res_h"], r["res_w"] = rh, rw
        r["win_x"], r["win_y"], r["out_w"], r["out_h"] = st["win"]
        r["dst_row_bytes"], r["filter"], r["flip"] = 3 * st["win"][2], st["filter"], st["flip"]
    return rec


def _colour_records(stages):
    """One wv_colour_ops record per stage (n_ops = 0 where the stage has no chain): the image is what the stage writes."""
    rec = np.zeros(len(stages), dtype=COLOUR_DTYPE)
    for r, st in zip(rec, stages):
        r["h"], r["w"], r["row_bytes"] = st["win"][3], st["win"][2], 3 * st["win"][2]
        r["n_ops"] = len(st["colour"])
        for i, (kind, factor) in enumerate(st["colour"]):
            r["kind"][i], r["factor"][i] = COLOUR_KINDS[kind], factor
    return rec


class LazyImage(object):
    """Stands in for a PIL image in a sizing pipeline: answers like one, logs instead of resampling."""

    def __init__(self, img):
        if not isinstance(img, Image.Image):
            raise TypeError(f"sizing='device' pipelines start from a PIL image, got {type(img).__name__}")
        self.img = img
        self.ops = []
        self.size = img.size
        self.mode = img.mode

    def _log(self, op, size):
        out = LazyImage.__new__(LazyImage)
        out.img, out.ops, out.size, out.mode = self.img, self.ops + [op], size, self.mode
        return out

    def resize(self, size, resample=Image.BICUBIC, **kwargs):
        if kwargs.get("box") is not None or kwargs.get("reducing_gap") is not None:
            raise ValueError("LazyImage.resize: box / reducing_gap are not recorded")
        if int(resample) not in _FILTERS:
            raise ValueError(f"LazyImage.resize: only BILINEAR and BICUBIC are recorded, got resample={resample}")
        size = (int(size[0]), int(size[1]))
        return self._log(("resize", size, _FILTERS[int(resample)]), size)

    def crop(self, box):
        x0, y0, x1, y1 = (int(round(v)) for v in box)
        return self._log(("crop", (x0, y0, x1 - x0, y1 - y0)), (x1 - x0, y1 - y0))

    def transpose(self, method):
        if method != Image.FLIP_LEFT_RIGHT:
            raise ValueError("LazyImage.transpose: only FLIP_LEFT_RIGHT is recorded")
        return self._log(("mirror",), self.size)

    def colour(self, kind, factor):
        """Record one colour operation: kind 'brightness', 'contrast', 'saturation' or 'hue', factor as ImageEnhance (and
        torchvision's adjust_hue) take it."""
        if kind not in _ENHANCERS and kind != "hue":
            raise ValueError(f"LazyImage.colour: unknown operation {kind!r}")
        return self._log(("colour", kind, float(factor)), self.size)

    def materialize(self):
        """The PIL image the log describes: the same calls on the real image (the oracle of the recorded stages)."""
        img = self.img
        for op in self.ops:
            if op[0] == "resize":
                img = img.resize(op[1], op[2])
            elif op[0] == "crop":
                x, y, w, h = op[1]
                img = img.crop((x, y, x + w, y + h))
            elif op[0] == "colour":
                img = pil_colour(img, op[1], op[2])
            else:
                img = img.transpose(Image.FLIP_LEFT_RIGHT)
        return img

    def to_item(self):
        try:
            stages = stages_from_ops(self.img.size[0], self.img.size[1], self.ops) if self.mode == "RGB" else None
        except NotRecordable:
            stages = None
        if stages is not None:
            rec, col = _records(stages), _colour_records(stages)
            rc = 0
            for table, r in ((STAGES, rec), (COLOURS, col)):
                for i in range(len(r)):                     # one record per launch: each on its own
                    rc = rc or table.check(r[i:i + 1])
                if rc != 0:
                    break
            if rc == 0:
                return RawItem(torch.from_numpy(np.array(self.img)), rec, col if col["n_ops"].any() else None)
            if rc != _lib.WV_ENOTSUP:
                _lib.check(rc, table.check_name)
        arr = np.array(self.materialize())                  # outside the kernel: PIL in the worker, as sizing="host" does
        if arr.ndim != 3 or arr.shape[2] < 3 or arr.dtype != np.uint8:
            raise ValueError(f"expected an 8-bit RGB image (H, W, 3), got array of shape {arr.shape} and dtype {arr.dtype}")
        return RawItem(torch.from_numpy(np.ascontiguousarray(arr[:, :, :3])), np.zeros(0, dtype=STAGE_DTYPE))


class RawItem(object):
    """What a worker returns for one image: ``pixels`` uint8 [h, w, 3] as decoded, ``stages`` its wv_size_stage records
    (offsets 0, tight rows; empty = the pixels are final), ``colour`` None or one wv_colour_ops record per stage: the chain
    that runs on what the stage wrote (n_ops = 0: none)."""

    def __init__(self, pixels, stages, colour=None):
        self.pixels = pixels
        self.stages = stages
        self.colour = colour

    @property
    def out_hw(self):
        if len(self.stages):
            return int(self.stages[-1]["out_h"]), int(self.stages[-1]["out_w"])
        return int(self.pixels.shape[0]), int(self.pixels.shape[1])


class RawBatch(object):
    """A collated batch of RawItems.
    data      uint8 [bytes]: the decoded images back to back (16-byte aligned starts)
    desc      int32 [records, 20]: wv_size_stage records, all of stage index 0 first, then all of stage index 1, ...
    launches  ((first record, records, max_out_h, max_out_w, max_ksize), ...) one entry per stage index
    out_shape (B, H, W); work_bytes: the device buffer size_images allocates -- the B sized images first, then the
              intermediate images of pipelines with more than one resample.
    Stage 0 reads ``data``; later stages read the work buffer.  Every image's last stage writes its slot of the result.
    colour          None, or int32 [records, 12]: wv_colour_ops records (bit patterns; the factors are fp32), grouped by
                    stage index like ``desc``; only images that have a chain on that stage are listed
    colour_launches () or one (first record, records, max_h, max_w) per stage index, records = 0 where no image has a chain:
                    the wv_colour_jitter call that follows the stage's wv_image_size launch, in place on the work buffer."""

    def __init__(self, data, desc, launches, out_shape, work_bytes, colour=None, colour_launches=()):
        self.data, self.desc, self.launches, self.out_shape, self.work_bytes = data, desc, tuple(launches), tuple(out_shape), work_bytes
        self.colour, self.colour_launches = colour, tuple(colour_launches)

    def __len__(self):
        return self.out_shape[0]

    @property
    def is_cuda(self):
        return self.data.is_cuda

    @property
    def device(self):
        return self.data.device

    def _moved(self, fn):
        return RawBatch(fn(self.data), fn(self.desc), self.launches, self.out_shape, self.work_bytes,
                        None if self.colour is None else fn(self.colour), self.colour_launches)

    def pin_memory(self):
        return self._moved(lambda t: t.pin_memory())

    def cuda(self, device=None, non_blocking=False):
        return self._moved(lambda t: t.cuda(device, non_blocking=non_blocking))

    def to(self, device, non_blocking=False):
        return self._moved(lambda t: t.to(device, non_blocking=non_blocking))


def _grouped(table, groups, maxima):
    """groups[s]: the records of stage index s, a list of one-record arrays -> (the table's tensor of all of them, stage
    index by stage index; one launch tuple per stage index: (first record, records, one maximum per entry of `maxima` -- a
    field name, or a function of the group's records), all zero behind `first` where the group is empty).  Every group
    passes the table's check here, on the host copy.  No record at all: (None, ())."""
    if not any(groups):
        return None, ()
    launches, first, chunks = [], 0, []
    for group in groups:
        if not group:
            launches.append((first, 0) + (0,) * len(maxima))
            continue
        g = np.concatenate(group)
        table.require(g)
        launches.append((first, len(g)) + tuple(int(g[m].max()) if isinstance(m, str) else m(g) for m in maxima))
        first += len(g)
        chunks.append(g)
    return table.tensor(chunks), launches


def _max_ksize(g):
    return max(max(ksize(int(r["crop_w"]), int(r["res_w"]), int(r["filter"])),
                   ksize(int(r["crop_h"]), int(r["res_h"]), int(r["filter"]))) for r in g)


def pack(items):
    """list of RawItem -> RawBatch (host tensors).  The packed descriptors pass wv_image_size_check (and the colour
    descriptors wv_colour_jitter_check) here, on the host copy: the device entry points cannot read them."""
    if not items:
        raise ValueError("raw_collate: empty batch")
    H, W = items[0].out_hw
    for it in items:
        if it.out_hw != (H, W):
            raise ValueError(f"raw_collate: images of one batch must be sized alike, got {it.out_hw} and {(H, W)}")
    B = len(items)
    recs = [it.stages if len(it.stages) else _records([_fresh_stage(*it.out_hw[::-1])]) for it in items]
    data_off, total = [], 0
    for it in items:
        data_off.append(total)
        total = _align(total + it.pixels.numel())
    data = torch.empty(total, dtype=torch.uint8)
    for it, off in zip(items, data_off):
        data[off:off + it.pixels.numel()] = it.pixels.reshape(-1)
    work = _align(B * H * W * 3)
    per_stage, colour_per_stage = [], []
    for i, rec in enumerate(recs):
        src = data_off[i]
        for s in range(len(rec)):
            r = rec[s:s + 1].copy()
            r["src_offset"] = src
            if s == len(rec) - 1:
                r["dst_offset"] = i * H * W * 3
            else:
                r["dst_offset"] = src = work
                work = _align(work + int(r["out_h"][0]) * int(r["dst_row_bytes"][0]))
            while len(per_stage) <= s:
                per_stage.append([])
                colour_per_stage.append([])
            per_stage[s].append(r)
            col = items[i].colour
            if col is not None and len(items[i].stages) and int(col["n_ops"][s]):
                c = col[s:s + 1].copy()                     # the image the stage wrote: same place, same pitch
                c["offset"], c["h"], c["w"], c["row_bytes"] = r["dst_offset"], r["out_h"], r["out_w"], r["dst_row_bytes"]
                colour_per_stage[s].append(c)
    desc, launches = _grouped(STAGES, per_stage, ("out_h", "out_w", _max_ksize))
    colour, colour_launches = _grouped(COLOURS, colour_per_stage, ("h", "w"))
    return RawBatch(data, desc, launches, (B, H, W), work, colour, colour_launches)


def raw_collate(batch):
    """collate_fn of a DataLoader over a dataset whose transform was built with sizing="device": RawItems become one
    RawBatch, everything else goes through torch's default collate (dict items key by key, like the default)."""
    from torch.utils.data import default_collate
    first = batch[0]
    if isinstance(first, RawItem):
        return pack(list(batch))
    if isinstance(first, Mapping):
        return {k: raw_collate([b[k] for b in batch]) for k in first}
    if isinstance(first, (tuple, list)) and any(isinstance(v, RawItem) for v in first):
        return type(first)(raw_collate(list(col)) for col in zip(*batch))
    return default_collate(batch)
