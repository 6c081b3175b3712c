"""The reference's export for the audio-visual sets, on the device: 8-bit maps to the ``.jpg`` files it writes and to the pixels it
reads back from them (csrc/jpeg_export.hip, arithmetic in include/diffsal.h "JPEG export").  For AVAD, Coutrot, DIEM, ETMD and
SumMe R/diffusion_trainer.py:898-935 (``save_img(..., av_data=True)``) does not write a PNG but ``pred_sal_%06d.jpg`` with
``cv2.imwrite``, and the benchmark scores what a decoder makes of that file:

* ``encode`` gives the complete files of a batch in device memory, ``save_predictions`` writes them; only finished file bytes
  travel to the host;
* ``roundtrip`` gives the decoded pixels in one launch, without the entropy coder: what scoring needs
  (``postprocess.protocol_metrics(..., quantize="jpeg")``);
* ``quant_table`` is libjpeg's table for a quality, on the host.

The file is 8-bit greyscale, baseline, libjpeg's slow-integer DCT, the standard tables unoptimised, quality 95 by default: every
step is integer arithmetic, so the result is a matter of bits, not of tolerance.  The tests hold the files and the decoded pixels
to Pillow 12.2 (libjpeg-turbo) byte for byte.  One thing could not be run where this module was written and rests on reading the
sources:

* OpenCV itself.  The claim is that ``cv2.imwrite(path, u8)`` of a 2-D uint8 array sets quality 95, no optimised tables, no
  progressive mode and libjpeg's defaults otherwise into the same libjpeg-turbo, and so writes the same scan and tables as Pillow's
  ``save(f, "JPEG", quality=95)``, and that ``cv2.imread`` decodes with libjpeg's default slow-integer inverse DCT.

GPU only: CPU tensors raise.
"""
from __future__ import annotations

import os
from typing import Sequence

import numpy as np
import torch

from . import ops

Tensor = torch.Tensor

# ITU-T T.81 Annex K.1, luminance, natural order
_BASE_Q = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
           103, 99)


def _quality(quality) -> int:
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f"jpeg: quality must be an integer in 1..100, got {quality!r}")
    return q


def quant_table(quality: int = 95) -> np.ndarray:
    """libjpeg's quantisation table for ``quality`` (``jpeg_quality_scaling``, baseline): int64 ``[64]`` in natural order."""
    q = _quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.asarray(_BASE_Q, dtype=np.int64) * s + 50) // 100, 1, 255)


def _maps(u8: Tensor, what: str = "u8") -> Tensor:
    """[B, 1, H, W] or [B, H, W] uint8 GPU tensor -> contiguous [B, H, W]"""
    if not isinstance(u8, Tensor) or not u8.is_cuda:
        raise RuntimeError(f"diff_sal_amd jpeg runs on the GPU only (no CPU fallback); {what} is on "
                           f"{getattr(u8, 'device', type(u8).__name__)}")
    if u8.dtype != torch.uint8:
        raise ValueError(f"jpeg: {what} must be uint8 (postprocess.to_uint8 gives it), got {u8.dtype}")
    if u8.dim() == 4 and u8.shape[1] == 1:
        u8 = u8[:, 0]
    if u8.dim() != 3 or u8.numel() == 0:
        raise ValueError(f"jpeg: {what} must be a non-empty [B, 1, H, W] or [B, H, W], got {tuple(u8.shape)}")
    if max(u8.shape[1:]) > 65535:
        raise ValueError(f"jpeg: {tuple(u8.shape[1:])}: a JPEG axis holds at most 65535 pixels")
    return u8.contiguous()


def capacity(h: int, w: int) -> int:
    """The bytes no file of an ``h x w`` image exceeds: the width of ``encode``'s rows."""
    return ops.jpeg_capacity(h, w)


def encode(u8: Tensor, quality: int = 95, return_decoded: bool = False):
    """The ``.jpg`` file of every image of ``u8`` (uint8 ``[B, H, W]``): ``(data uint8 [B, cap], lengths int32 [B])`` on the device,
    image ``b``'s file being ``data[b, :lengths[b]]`` (the bytes behind it are undefined).  ``return_decoded=True`` adds what a
    decoder reads back from those files, uint8 ``[B, H, W]``.  No host copy, no synchronisation: capturable."""
    q = _quality(quality)
    data, lengths, recon = ops.jpeg_encode(_maps(u8), q, want_recon=bool(return_decoded))
    return (data, lengths, recon) if return_decoded else (data, lengths)


def roundtrip(u8: Tensor, quality: int = 95) -> Tensor:
    """What a decoder reads back from ``encode(u8, quality)``'s files, uint8 ``[B, H, W]``, without making them: one launch."""
    return ops.jpeg_roundtrip(_maps(u8), _quality(quality))


def save_predictions(pred: Tensor, video_ids: Sequence, frame_ids: Sequence, root: str, quality: int = 95):
    """The reference's ``save_img`` for the audio-visual sets: ``<root>/<video id>/pred_sal_{frame id:06d}.jpg`` holding
    ``encode(postprocess.to_uint8(pred))``'s bytes.  One host copy of ``lengths``, then one of the used part of ``data``: nothing else leaves the device.  The
    reference also renames the data set's folder inside the video id (``"AVAD/..."`` -> ``"avad/..."``); that is left to the caller,
    who passes the ids as the folders should be named.  Returns the paths written."""
    from . import postprocess

    q = _quality(quality)
    u8 = postprocess.to_uint8(pred)
    frame_ids = [int(f) for f in (frame_ids.reshape(-1).tolist() if isinstance(frame_ids, Tensor) else frame_ids)]
    video_ids = list(video_ids)
    if not (u8.shape[0] == len(video_ids) == len(frame_ids)):
        raise ValueError(f"jpeg: {u8.shape[0]} predictions, {len(video_ids)} video ids, {len(frame_ids)} frame ids")
    data, lengths = encode(u8, q)
    n = lengths.cpu().numpy()
    host = data[:, :int(n.max())].cpu().numpy()      # the rows cut at the longest file: a few per cent of their capacity
    paths = []
    for row, length, vid, fid in zip(host, n, video_ids, frame_ids):
        d = os.path.join(root, str(vid))
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"pred_sal_{fid:06d}.jpg")
        with open(path, "wb") as f:
            f.write(row[:int(length)].tobytes())
        paths.append(path)
    return paths
