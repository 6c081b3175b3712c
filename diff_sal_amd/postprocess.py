"""From the sampler's map to the map the benchmark scores, on the device: the 8-bit export, the float map read back from it and
the spline resize to the annotation's resolution (csrc/postprocess.hip, arithmetic in include/diffsal.h "benchmark
post-processing").  The reference scores what it wrote to disk, not the tensor the sampler returned:

* R/diffusion_trainer.py:898-935 quantises each prediction with ``normalize_data`` (R/util/utils.py:11-16) and writes a PNG:
  ``to_uint8`` gives those bytes, ``save_predictions`` the files;
* R/compute_metrics.py:9-26 reads the PNG back with ``plt.imread``, float32 = byte / 255: ``from_uint8``;
* R/metrics/metrics.py:41-42,102-103,195-196,218-219,243-244 resizes that map to the annotation's shape with skimage
  ``resize``, ``order=3, mode='reflect'`` for the AUCs, CC and SIM and the default ``order=1`` for NSS: ``resize``;
* ``protocol_metrics`` chains the three in front of ``eval_metrics.benchmark_metrics`` without a host copy or a synchronisation.

``resize`` computes ``scipy.ndimage.zoom(map, (H / h, W / w), order=order, mode='mirror', grid_mode=True)`` in float64 from the
float32 input, clamps to the input's range (``clip``) and rounds once to float32; the tests hold it to scipy 1.15 to 1e-12
before that rounding.  Two things could not be run where this module was written and rest on reading the sources:

* skimage itself.  The claim is that skimage (>= 0.19) executes exactly that zoom call for an upscale and then clips, and that
  for a target shorter than the map on some axis it first runs ``scipy.ndimage.gaussian_filter(map, sigma, mode='mirror')`` with
  ``sigma = max(0, (in / out - 1) / 2)`` per axis, zooms the filtered map and clips to the range of the map as it came.  That
  downscale is opt-in: ``resize(..., anti_aliasing=True)``, ``antialias`` for the Gaussian alone (held bit-equal to scipy's
  float32 result), ``gaussian_weights`` for its table; without the keyword a downscale raises as before.
* the reference's JPEG path.  For the audio-visual sets it writes ``pred_sal_%06d.jpg`` with ``cv2.imwrite``.  That export is integer
  arithmetic throughout and lives in ``diff_sal_amd.jpeg`` (files and read-back pixels, held to Pillow byte for byte; its docstring
  says what rests on reading OpenCV's sources): ``protocol_metrics(..., quantize="jpeg")`` scores the map a decoder reads back from
  that file, ``jpeg.save_predictions`` writes the files.  ``save_predictions`` here writes PNG only, in the layout of the visual sets,
  through Pillow on the host; ``png.save_predictions`` writes the same layout from files encoded on the device (``png.encode``).

Deliberate definition: a flat prediction (max == min; ``normalize_data`` divides by zero there) quantises to all zeros.
GPU only: CPU tensors raise.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _image_files
from . import eval_metrics as _em
from . import ops

Tensor = torch.Tensor


def _map3(t: Tensor, what: str, floating: bool = True) -> Tensor:
    """[B, 1, H, W] or [B, H, W] GPU tensor -> [B, H, W]"""
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise RuntimeError(f"diff_sal_amd postprocess runs on the GPU only (no CPU fallback); {what} is on "
                           f"{getattr(t, 'device', type(t).__name__)}")
    if floating and not t.is_floating_point():
        raise ValueError(f"postprocess: {what} must be a floating map, got {t.dtype}")
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError(f"postprocess: {what} must be a non-empty [B, 1, H, W] or [B, H, W], got {tuple(t.shape)}")
    return t


def to_uint8(pred: Tensor) -> Tensor:
    """``normalize_data`` per image, bit for bit in float32: uint8 ``[B, H, W]``."""
    p = _map3(pred, "pred")
    B, H, W = p.shape
    u8, _ = ops.map_to_u8(p.reshape(B, -1).float().contiguous())
    return u8.view(B, H, W)


def from_uint8(u8: Tensor) -> Tensor:
    """What ``plt.imread`` returns for the 8-bit PNG: float32 byte / 255, ``[B, H, W]``."""
    q = _map3(u8, "u8", floating=False)
    if q.dtype != torch.uint8:
        raise ValueError(f"postprocess: u8 must be uint8, got {q.dtype}")
    return ops.map_from_u8(q.contiguous())


def _size(size) -> Tuple[int, int]:
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"postprocess: size must be (H, W), got {size!r}") from None
    return H, W


MAX_RADIUS = 64      # the anti-aliasing Gaussian's radius the kernels take (include/diffsal.h): sigma < 16, a factor below 33


def gaussian_weights(in_size: int, out_size: int) -> Optional[np.ndarray]:
    """The anti-aliasing Gaussian of one axis that goes from ``in_size`` to ``out_size`` samples, as skimage (>= 0.19) sets it and
    ``scipy.ndimage.gaussian_filter`` tabulates it: ``sigma = max(0, (in_size / out_size - 1) / 2)``, radius ``r = int(4 sigma +
    0.5)``, ``exp(-0.5 / sigma^2 * k^2)`` for ``k = -r .. r`` in float64, divided by their sum.  Returns the ``r + 1`` weights from
    the centre outwards (float64), or None where the axis does not shrink (``sigma <= 1e-15``: scipy skips the axis).  Computed with
    NumPy as scipy does: one ulp in a weight changes output bits."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"postprocess: gaussian_weights needs sizes of at least 1, got {in_size} -> {out_size}")
    sigma = max(0.0, (in_size / out_size - 1) / 2)
    if not sigma > 1e-15:
        return None
    r = int(4.0 * sigma + 0.5)
    if r > MAX_RADIUS:
        raise ValueError(f"postprocess: {in_size} -> {out_size} is a downscale by a factor of {in_size / out_size:.4g}: its anti-aliasing "
                         f"Gaussian has radius {r}, above the {MAX_RADIUS} (a factor below 33) the kernels are built for")
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    return np.ascontiguousarray(phi[r:])


def _weights(m: Tensor, H: int, W: int):
    if H < 1 or W < 1:
        raise ValueError(f"postprocess: size must be at least 1 x 1, got {(H, W)}")
    return gaussian_weights(m.shape[1], H), gaussian_weights(m.shape[2], W)


def antialias(map: Tensor, size) -> Tensor:
    """The Gaussian stage of an anti-aliased ``resize`` of ``[B, h, w]`` maps to ``size``, alone: what
    ``scipy.ndimage.gaussian_filter(map, sigma, mode='mirror')`` returns for the float32 map with ``gaussian_weights``' sigma per
    axis, bit for bit (rows first, float64 sums, one rounding to float32 per axis).  An axis that does not shrink is left as it
    is.  float32 ``[B, h, w]``."""
    m = _map3(map, "map")
    wy, wx = _weights(m, *_size(size))
    return ops.map_gauss(m.float().contiguous(), wy, wx)


def resize(map: Tensor, size, *, order: int = 3, clip: bool = True, dtype: torch.dtype = torch.float32,
           anti_aliasing: bool = False) -> Tensor:
    """Spline resize of ``[B, H, W]`` maps to ``size = (H', W')``: ``order`` 3 (cubic B-spline) or 1 (linear), mirror boundary,
    ``clip`` to each image's input range.  float32; ``dtype=torch.float64`` returns the value before the last rounding (what the
    tests compare with scipy).  By default neither axis may be shorter than the input's: a downscale raises.
    ``anti_aliasing=True`` takes any size of at least 1 x 1 and follows skimage's default rule: if and only if some axis
    shrinks, the map first passes the Gaussian of ``antialias`` (on the shrinking axes), the spline reads the filtered float32 map,
    and the clip keeps the range of the map as it came.  Where no axis shrinks the result is the default call's, bit for bit."""
    m = _map3(map, "map")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"postprocess: dtype must be float32 or float64, got {dtype}")
    H, W = _size(size)
    if anti_aliasing not in (True, False):
        raise ValueError(f"postprocess: anti_aliasing must be True or False, got {anti_aliasing!r}")
    if anti_aliasing and (H < m.shape[1] or W < m.shape[2]):
        wy, wx = _weights(m, H, W)
        return ops.map_resize_aa(m.float().contiguous(), H, W, wy, wx, order=order, clip=clip, out_f64=dtype == torch.float64)
    if H < m.shape[1] or W < m.shape[2]:
        raise ValueError(f"postprocess: resize {tuple(m.shape[1:])} -> {(H, W)} shrinks an axis; a downscale needs skimage's "
                         "anti-aliasing path: pass anti_aliasing=True")
    return ops.map_resize(m.float().contiguous(), H, W, order=order, clip=clip, out_f64=dtype == torch.float64)


def protocol_metrics(pred: Tensor, fix: Optional[Tensor], gt: Optional[Tensor] = None, other: Optional[Tensor] = None, *,
                     quantize=True, anti_aliasing: bool = False, **benchmark_metrics_kwargs) -> Dict[str, Tensor]:
    """The benchmark's numbers for the sampler's maps: quantise -> / 255 -> resize to the annotations' resolution when it differs
    -> ``eval_metrics.benchmark_metrics`` (whose keyword arguments pass through).  ``quantize="jpeg"`` is the audio-visual sets'
    protocol: quantise -> the pixels read back from the JPEG file of that map (``jpeg.roundtrip``, quality 95) -> / 255 -> the rest
    alike.  ``fix``, ``gt`` and ``other`` share one resolution, at least the prediction's on both axes unless ``anti_aliasing=True``,
    which ``resize`` then gets (annotations shorter than the prediction on some axis: skimage's Gaussian first).  As in the reference, the map NSS scores is resized with order 1 and the
    map of the other metrics with order 3: when both kinds are asked for and the shapes differ, ``benchmark_metrics`` runs twice.
    ``quantize=False`` scores the float map as it is.  ``{name: [B] float64}``; no host copy, no synchronisation: capturable."""
    p = _map3(pred, "pred")
    B, h, w = p.shape
    if isinstance(quantize, str) and quantize == "jpeg":
        from . import jpeg

        p = from_uint8(jpeg.roundtrip(to_uint8(p)))
    elif isinstance(quantize, str) or quantize not in (True, False):
        raise ValueError(f"postprocess: quantize must be True, False or 'jpeg', got {quantize!r}")
    elif quantize:
        _, f = ops.map_to_u8(p.reshape(B, -1).float().contiguous(), want_u8=False, want_float=True)
        p = f.view(B, h, w)
    target = None
    for t, what in ((fix, "fix"), (gt, "gt"), (other, "other")):
        if t is None:
            continue
        s = tuple(_map3(t, what, floating=False).shape)
        if target is not None and s != target:
            raise ValueError(f"postprocess: {what} {s} does not share the resolution of the other annotations {target}")
        target = s
    if target is None:
        raise ValueError("postprocess: protocol_metrics needs at least one annotation map")
    kw = dict(benchmark_metrics_kwargs)
    if target == (B, h, w):
        return _em.benchmark_metrics(p, fix, gt, other, **kw)
    if target[0] != B:
        raise ValueError(f"postprocess: {target[0]} annotation maps for {B} predictions")
    want = set(_em.METRICS if kw.get("metrics") is None else kw.pop("metrics"))
    kw.pop("metrics", None)
    if not want <= set(_em.METRICS):
        raise ValueError(f"postprocess: unknown metric(s) {sorted(want - set(_em.METRICS))}; choose from {_em.METRICS}")
    if fix is None:
        want -= {"auc_judd", "auc_borji", "auc_shuffled", "nss"}
    if gt is None:
        want -= {"cc", "sim"}
    if other is None:
        want -= {"auc_shuffled"}
    if not want:
        raise ValueError("postprocess: the inputs given allow none of the metrics asked for")
    res: Dict[str, Tensor] = {}
    cubic = tuple(k for k in _em.METRICS if k in want and k != "nss")
    if cubic:
        res.update(_em.benchmark_metrics(resize(p, target[1:], order=3, anti_aliasing=anti_aliasing), fix, gt, other, metrics=cubic, **kw))
    if "nss" in want:
        res.update(_em.benchmark_metrics(resize(p, target[1:], order=1, anti_aliasing=anti_aliasing), fix, metrics=("nss",)))
    return {k: res[k] for k in _em.METRICS if k in res}


def save_predictions(pred: Tensor, video_ids: Sequence, frame_ids: Sequence, root: str, *, fmt: str = "png"):
    """The reference's ``save_img`` for the visual sets: ``<root>/<video id>/<frame id>.png`` holding ``to_uint8``'s bytes as an
    8-bit greyscale PNG.  Only the bytes travel to the host, where Pillow encodes one file after the other;
    ``diff_sal_amd.png.save_predictions`` encodes on the device and writes the same layout (the same pixels, other file bytes).
    Returns the paths written."""
    if fmt != "png":
        raise ValueError(f"postprocess: fmt {fmt!r} is not offered (the reference's JPEG for the audio-visual sets is lossy: "
                         "a map written that way is not this one; diff_sal_amd.jpeg.save_predictions writes those files); use 'png'")
    from PIL import Image

    u8 = to_uint8(pred)
    video_ids, frame_ids = _image_files.checked_ids(u8.shape[0], video_ids, frame_ids, "postprocess")
    paths = _image_files.prediction_paths(root, video_ids, frame_ids, "{}.png")
    for img, path in zip(u8.cpu().numpy(), paths):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        Image.fromarray(img).save(path, format="PNG")      # 2-D uint8: mode "L"
    return paths
