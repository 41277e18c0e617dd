"""Image preparation of a KITTI batch on the GPU (``dataset.device_aug``; include/monosowa_image.h, csrc/image_prep.hip).

In this mode the loader's workers only decode the PNG and draw the augmentation; the pixels -- photometric distortion,
flip, PIL's affine bilinear resampling to the network's resolution, normalisation, HWC -> CHW -- are one HIP launch per
batch, bit for bit equal to what ``KITTI_Dataset.__getitem__`` computes on the CPU:

    make_record(size, trans_inv, flipped, pd)   one image's parameter record, float64 [RECORD_DOUBLES]  (info["prep"])
    collate_raw(samples)                        pads the raw uint8 images of a batch to one canvas, default-collates the rest
    is_raw_batch(inputs)                        a collated raw batch (uint8 [B, Hc, Wc, 3]) rather than prepared images
    prepare(raw, records, device, out=None)     -> float32 [B, 3, H, W], channels-last on the GPU (what stage_batch produces)
    prepare_reference(raw, records)             the same in numpy: float64 coordinates and PIL's rules, photometric.py's float32

``prepare`` on a CPU device IS ``prepare_reference``; on a GPU a missing library is an error, never a fall-back.
"""
import ctypes
import os

import numpy as np
import torch

from . import photometric

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libmonosowa_image.so")
SYMBOLS = ("mono_image_record_doubles", "mono_image_prep_f32")
_lib = None

RECORD_DOUBLES = 16
FLIP, PD, BRIGHTNESS, CONTRAST_FIRST, CONTRAST, SATURATION, HUE, PERMUTE = 1, 2, 4, 8, 16, 32, 64, 128     # monosowa_image.h
RESOLUTION = (1280, 384)                                                  # W, H of KITTI_Dataset
MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(_PATH):
            raise RuntimeError("HIP extension %s is missing: run `python -m monosowa_amd.build`" % _PATH)
        lib = ctypes.CDLL(_PATH)
        P, I = ctypes.c_void_p, ctypes.c_int
        lib.mono_image_record_doubles.restype = I
        lib.mono_image_record_doubles.argtypes = []
        lib.mono_image_prep_f32.restype = I
        lib.mono_image_prep_f32.argtypes = [P] * 4 + [I] * 5 + [P]
        if lib.mono_image_record_doubles() != RECORD_DOUBLES:
            raise RuntimeError("record layout mismatch in %s" % _PATH)
        _lib = lib
    return _lib


def make_record(size, trans_inv, flipped, pd=None):
    """One image's record (layout: include/monosowa_image.h).  ``size`` = (w, h) of the decoded image, ``trans_inv`` the 2 x 3
    output -> input matrix the CPU path hands to ``Image.transform``, ``pd`` a ``PhotometricDistort.draw()`` dict or None."""
    rec = np.zeros(RECORD_DOUBLES, dtype=np.float64)
    rec[0], rec[1] = int(size[0]), int(size[1])
    rec[2:8] = np.asarray(trans_inv, dtype=np.float64).reshape(-1)
    flags = FLIP if flipped else 0
    if pd is not None:
        flags |= PD | (CONTRAST_FIRST if pd["contrast_first"] else 0)
        for key, bit, slot in (("brightness", BRIGHTNESS, 9), ("contrast", CONTRAST, 10), ("saturation", SATURATION, 11), ("hue", HUE, 12)):
            if pd[key] is not None:
                flags |= bit
                rec[slot] = np.float32(pd[key])                            # enters the float32 arithmetic as float32(draw)
        if pd["perm"] is not None:
            flags |= PERMUTE
            rec[13] = photometric._PERMS.index(tuple(pd["perm"]))
    rec[8] = flags
    return rec


def record_pd(rec):
    """The photometric part of a record back as a ``PhotometricDistort.draw()`` dict (None: aug_pd off)."""
    flags = int(rec[8])
    if not flags & PD:
        return None
    val = lambda bit, slot: float(rec[slot]) if flags & bit else None
    return {"brightness": val(BRIGHTNESS, 9), "contrast_first": bool(flags & CONTRAST_FIRST), "contrast": val(CONTRAST, 10),
            "saturation": val(SATURATION, 11), "hue": val(HUE, 12), "perm": photometric._PERMS[int(rec[13])] if flags & PERMUTE else None}


def collate_raw(samples):
    """Collate function of the raw mode: the images ``[h, w, 3]`` uint8 (sizes may differ inside a batch) go to the top-left
    corner of one zero canvas ``[B, Hc, Wc, 3]`` (the records in ``info["prep"]`` keep each true size; the padding is never
    read), everything else is default-collated.  The ``test`` split's third entry (the image again) becomes the same canvas."""
    from torch.utils.data import default_collate
    raws = [s[0] for s in samples]
    canvas = torch.zeros((len(raws), max(r.shape[0] for r in raws), max(r.shape[1] for r in raws), 3), dtype=torch.uint8)
    for i, r in enumerate(raws):
        canvas[i, :r.shape[0], :r.shape[1]] = torch.from_numpy(np.ascontiguousarray(r))
    image_again = all(s[2] is s[0] for s in samples)
    rest = default_collate([(s[1], s[3]) if image_again else tuple(s[1:]) for s in samples])
    return (canvas, rest[0], canvas, rest[1]) if image_again else (canvas,) + tuple(rest)


def is_raw_batch(inputs):
    return torch.is_tensor(inputs) and inputs.dtype == torch.uint8 and inputs.dim() == 4 and inputs.shape[-1] == 3


def normalisation_table(mean=MEAN, std=STD):
    """lut[u, c] = (u / 255 - mean[c]) / std[c] in float32 exactly as numpy evaluates the CPU path's expression."""
    u = np.arange(256, dtype=np.uint8)[:, None].astype(np.float32)
    return np.ascontiguousarray((u / 255.0 - np.asarray(mean, np.float32)) / np.asarray(std, np.float32), dtype=np.float32)


def affine_bilinear(src, a, size):
    """``Image.fromarray(src).transform(size, Image.AFFINE, a, Image.BILINEAR)`` restated in float64 numpy (Pillow's
    ImagingGenericTransform with affine_transform and bilinear_filter32RGB): src uint8 [h, w, 3] -> uint8 [H, W, 3]."""
    h, w = src.shape[:2]
    W, H = size
    X, Y = np.meshgrid(np.arange(W, dtype=np.float64) + 0.5, np.arange(H, dtype=np.float64) + 0.5)
    xin = a[0] * X + a[1] * Y + a[2]
    yin = a[3] * X + a[4] * Y + a[5]
    inside = (xin >= 0.0) & (xin < w) & (yin >= 0.0) & (yin < h)
    xin, yin = xin - 0.5, yin - 0.5
    x, y = np.floor(xin), np.floor(yin)
    dx, dy = (xin - x)[..., None], (yin - y)[..., None]
    with np.errstate(invalid="ignore"):
        x, y = x.astype(np.int64), y.astype(np.int64)
    x0, x1, y0 = np.clip(x, 0, w - 1), np.clip(x + 1, 0, w - 1), np.clip(y, 0, h - 1)
    s = src.astype(np.float64)
    v1 = s[y0, x0] + (s[y0, x1] - s[y0, x0]) * dx
    below = (y + 1 >= 0) & (y + 1 < h)
    y1 = np.where(below, y + 1, 0)
    v2 = np.where(below[..., None], s[y1, x0] + (s[y1, x1] - s[y1, x0]) * dx, v1)
    out = np.floor(v1 + (v2 - v1) * dy).astype(np.uint8)                   # (UINT8) v of a non-negative v: truncated, not rounded
    out[~inside] = 0                                                      # PIL's fill
    return out


def prepare_reference(raw, records, resolution=RESOLUTION, mean=MEAN, std=STD):
    """numpy restatement of the whole chain: raw uint8 ``[B, Hc, Wc, 3]`` + records ``[B, RECORD_DOUBLES]`` -> float32
    ``[B, 3, H, W]`` (one image ``[h, w, 3]`` + one record -> ``[3, H, W]``).  Tensors or arrays in, an array out."""
    raw = raw.cpu().numpy() if torch.is_tensor(raw) else np.asarray(raw)
    records = records.cpu().numpy() if torch.is_tensor(records) else np.asarray(records, dtype=np.float64)
    if raw.ndim == 3:
        return prepare_reference(raw[None], records[None], resolution, mean, std)[0]
    _check(raw, records)
    lut = normalisation_table(mean, std)
    out = np.empty((raw.shape[0], 3, resolution[1], resolution[0]), dtype=np.float32)
    for i, rec in enumerate(records):
        src = raw[i, :int(rec[1]), :int(rec[0])]
        pd = record_pd(rec)
        if pd is not None:
            src = photometric.wrap_to_uint8(photometric.PhotometricDistort.apply(src, pd))
        if int(rec[8]) & FLIP:
            src = src[:, ::-1]                                            # (the kernel folds this into the column index)
        u8 = affine_bilinear(src, rec[2:8], resolution)
        for c in range(3):
            out[i, c] = lut[u8[..., c], c]
    return out


def _check(raw, records):
    if raw.dtype not in (np.uint8, torch.uint8) or raw.ndim != 4 or raw.shape[-1] != 3:
        raise ValueError("raw images must be uint8 [B, Hc, Wc, 3], got %s %s" % (raw.dtype, tuple(raw.shape)))
    if tuple(records.shape) != (raw.shape[0], RECORD_DOUBLES) or records.dtype not in (np.float64, torch.float64):
        raise ValueError("records must be float64 [%d, %d], got %s %s" % (raw.shape[0], RECORD_DOUBLES, records.dtype, tuple(records.shape)))
    if not (torch.is_tensor(records) and records.is_cuda):               # host records: sizes inside the canvas (the kernel clamps too)
        w, h = records[:, 0], records[:, 1]
        if bool((w < 1).any()) or bool((h < 1).any()) or bool((w > raw.shape[2]).any()) or bool((h > raw.shape[1]).any()):
            raise ValueError("a record's image size lies outside the canvas %d x %d" % (raw.shape[2], raw.shape[1]))


_LUTS = {}


def _device_lut(device, mean, std):
    key = (device, np.asarray(mean, np.float32).tobytes(), np.asarray(std, np.float32).tobytes())
    if key not in _LUTS:
        _LUTS[key] = torch.from_numpy(normalisation_table(mean, std)).to(device)
    return _LUTS[key]


def prepare(raw, records, device, resolution=RESOLUTION, mean=MEAN, std=STD, out=None):
    """raw uint8 ``[B, Hc, Wc, 3]`` and records float64 ``[B, RECORD_DOUBLES]`` (host tensors, pinned or not, or already on
    ``device``) -> the float32 batch ``[B, 3, H, W]`` on ``device``: channels-last from one launch of the library on the
    current stream after non-blocking copies, with no device -> host synchronisation; on a CPU device, ``prepare_reference``.
    ``out``: a float32 ``[B, 3, H, W]`` tensor on ``device`` (channels-last on a GPU) to write into instead of allocating -- the
    static input of a captured graph; it is returned."""
    device = torch.device(device)
    if out is not None:
        want = (raw.shape[0], 3, resolution[1], resolution[0])
        if out.dtype != torch.float32 or tuple(out.shape) != want or out.device.type != device.type \
                or (device.type == "cuda" and not out.is_contiguous(memory_format=torch.channels_last)):
            raise ValueError("out must be a float32 %s tensor on %s (channels-last on a GPU), got %s %s on %s"
                             % (want, device, out.dtype, tuple(out.shape), out.device))
    if device.type != "cuda":
        res = torch.from_numpy(prepare_reference(raw, records, resolution, mean, std))
        return res if out is None else out.copy_(res)
    _check(raw, records)
    if resolution[0] % 4:
        raise ValueError("the output width must be a multiple of 4, got %d" % resolution[0])
    from ._lib import on_device, raw_stream
    B, Hc, Wc = raw.shape[0], raw.shape[1], raw.shape[2]
    with on_device(device):
        lut = _device_lut(torch.device("cuda", torch.cuda.current_device()), mean, std)
        raw = raw.to(device, non_blocking=True).contiguous()
        records = records.to(device, non_blocking=True).contiguous()
        if out is None:
            out = torch.empty((B, 3, resolution[1], resolution[0]), dtype=torch.float32, device=device, memory_format=torch.channels_last)
        code = load().mono_image_prep_f32(raw.data_ptr(), records.data_ptr(), lut.data_ptr(), out.data_ptr(), B, Hc, Wc,
                                          resolution[1], resolution[0], raw_stream())
    if code:
        raise RuntimeError("mono_image_prep_f32 failed with code %d" % code)
    return out
