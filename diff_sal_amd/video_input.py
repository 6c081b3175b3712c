"""From decoded uint8 frames in device memory to the ``img [B, 3, T, h, w]`` clip ``VideoSaliencyModel.forward`` hands to ``MViT``
(csrc/video_input.hip, arithmetic in include/diffsal.h "video front end").  The reference builds that tensor per clip on the host
with Pillow:

* R/datasets/saliency_db.py:29-36 (``pil_loader``) resizes every frame to 320 x 240 with ``Image.resize``'s default filter, which
  is bicubic;
* R/datasets/saliency_db.py:292-296 applies ``Scale(sample_size)`` (bilinear), ``ToTensor(norm_value)`` and
  ``Normalize(mean, std)``; :382-394 stacks the frames and permutes them;
* R/datasets/meta_data.py:27-35 and R/datasets/dhf1k_data.py:72-81 run ``transforms.Resize(img_size)`` on the PIL image
  (bilinear), ``ToTensor`` and ``Normalize``;
* the targets (``target_transform``, saliency_db.py:298-301; ``sal_transform``, meta_data.py:32-35) are the same resize of an 'L'
  image and ``/ 255``.

Sixteen-frame clips of neighbouring starts share fifteen frames, and the reference transforms each of them sixteen times.  Here a
video's frames are uploaded as uint8 and transformed once (``transform_frames``, which returns uint8 the caller may keep per
video); every clip is then a gather through a 256-entry look-up table per channel (``gather_clips``).

Pillow's 8-bit resample is integer arithmetic (22-bit fixed-point coefficients, an int32 accumulator, a uint8 image between the
horizontal and the vertical pass), and ``ToTensor`` / ``Normalize`` see only 256 different inputs per channel, so the result is
**bit-equal** to the reference's, not merely close.  The coefficient tables are built here in float64 as Pillow builds them
(``resample_table``); the look-up tables are built with the reference's own torch CPU operations (``normalize_table``).

JPEG decoding with ``convert('RGB' | 'L')`` is ``jpeg.decode`` / ``jpeg.decode_files``, whose output is the ``frames`` taken here; the
visual sets' PNG frames and maps are decoded the same way by ``png.decode`` / ``png.decode_files``.  Only the bilinear and bicubic filters are built; all
frames of a call share one source size, except in ``resize_groups`` / ``transform_groups`` / ``target_maps_groups``, which take one
tensor per source size (a shuffled training batch holds clips of several videos) and still make a fixed number of launches.  Indices given on the host (a sequence, a numpy array, a CPU tensor) are range-checked
here and uploaded; a GPU tensor is used as it is, with no host copy and no synchronisation (the kernel clamps what could not be
checked), so the call can be captured in a graph.  The first call for a size, filter or normalisation uploads its tables from
host memory, which a capture does not allow: call once, or ``warm(device, ...)``, before capturing.  GPU only: a CPU ``frames``
raises.
"""
from __future__ import annotations

import math
import statistics
from decimal import ROUND_HALF_UP, Decimal, localcontext
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, ops

Tensor = torch.Tensor

FILTERS = {"bilinear": ops.FILTER_BILINEAR, "bicubic": ops.FILTER_BICUBIC}
PRECISION_BITS = 22                                # Pillow: 32 - 8 - 2
PRE_SIZE = (240, 320)                              # pil_loader's new_size = (320, 240), as (h, w)
SAMPLE_SIZE = (224, 384)                           # R/cfgs/dataset.json sample_size [384, 224], as (h, w)
DATASET_NORM_VALUE = 1                             # R/cfgs/dataset.json
DATASET_MEAN = (114.7748, 107.7354, 99.475)
DATASET_STD = (38.7568578, 37.88248729, 40.02898126)
IMAGENET_MEAN = (0.485, 0.456, 0.406)              # R/datasets/meta_data.py:30, dhf1k_data.py
IMAGENET_STD = (0.229, 0.224, 0.225)


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x: float) -> float:
    # Keys' cubic with a = -0.5, in the operation order of Pillow's bicubic_filter
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_KERNELS = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0)}


def _filter_id(name: str) -> int:
    try:
        return FILTERS[name]
    except (KeyError, TypeError):
        raise ValueError(f"video_input: filter must be 'bilinear' or 'bicubic', got {name!r}") from None


def resample_table(in_size: int, out_size: int, filter: str = "bilinear") -> Tuple[np.ndarray, np.ndarray]:
    """``(bounds, kk)`` of one axis as Pillow's ``precompute_coeffs`` and ``normalize_coeffs_8bpc`` build them: ``bounds`` int32
    ``[out_size, 2]`` holds (first source index, tap count), ``kk`` int32 ``[out_size, ksize]`` the weights times 2^22, rounded
    half away from zero, zero past the count.  Python float is float64 and the operation order is Pillow's, so the integers are
    Pillow's."""
    _filter_id(filter)
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError(f"video_input: sizes must be positive, got {in_size} -> {out_size}")
    kernel, support0 = _KERNELS[filter]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = support0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for o in range(out_size):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), in_size) - xmin
        w = [kernel((t + xmin - center + 0.5) * ss) for t in range(count)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        bounds[o] = (xmin, count)
        for t, v in enumerate(w):
            kk[o, t] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
    return bounds, kk


def _cpu_channel(norm_value) -> Tensor:
    return torch.arange(256, dtype=torch.uint8).float().div(norm_value)


def normalize_table(norm_value=DATASET_NORM_VALUE, mean: Sequence[float] = DATASET_MEAN, std: Sequence[float] = DATASET_STD) -> Tensor:
    """float32 ``[3, 256]`` on the CPU: what ``ToTensor(norm_value)`` followed by ``Normalize(mean, std)`` makes of each byte value
    in each channel, computed with the reference's own torch CPU operations in its order (spatial_transforms.py:78 and :109-110):
    ``byte.float().div(norm_value)``, then per channel ``sub_(mean).div_(std)``.  ``normalize_table(255, IMAGENET_MEAN,
    IMAGENET_STD)`` is torchvision's ``ToTensor`` + ``Normalize`` of meta_data.py and dhf1k_data.py."""
    mean, std = [float(v) for v in mean], [float(v) for v in std]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("video_input: mean and std have three entries")
    rows = []
    for m, s in zip(mean, std):
        t = _cpu_channel(norm_value)
        t.sub_(m).div_(s)
        rows.append(t)
    return torch.stack(rows, 0).contiguous()


def target_table() -> Tensor:
    """float32 ``[1, 256]`` on the CPU: ``transforms.ToTensor`` of an 'L' image, ``byte.float().div(255)``."""
    return _cpu_channel(255)[None].contiguous()


# ---- the reference's index arithmetic (host) ---------------------------------------------------------------------------

def center_crop_indices(frame_indices: Sequence[int], size: int) -> list:
    """``TemporalCenterCrop(size)`` (R/datasets/temporal_transforms.py:34-53): the ``size`` indices around the middle of the list;
    a shorter list is padded by walking it again from its head (the walk reads what it appends, so it cycles)."""
    frame_indices = list(frame_indices)
    size = int(size)
    center = len(frame_indices) // 2
    begin = max(0, center - size // 2)
    end = min(begin + size, len(frame_indices))
    out = frame_indices[begin:end]
    for index in out:
        if len(out) >= size:
            break
        out.append(index)
    return out


def median_index(frame_indices: Sequence[int]) -> int:
    """The frame whose annotation labels the clip (R/datasets/saliency_db.py:369-372): the median of the indices, a half rounded
    up (``Decimal`` under ROUND_HALF_UP)."""
    with localcontext() as ctx:
        ctx.rounding = ROUND_HALF_UP
        return int(Decimal(statistics.median(list(frame_indices))).to_integral_value())


def dhf1k_indices(start: int, alternate: int = 1, len_snippet: int = 16) -> list:
    """The frame numbers of a DHF1K clip (R/datasets/dhf1k_data.py:70-74): ``start + alternate * i + 1`` for ``i`` below
    ``len_snippet``, which is capped at 16.  They are the reference's 1-based file numbers (``'%d.png'``); subtract one for a
    position in a tensor that holds the video from its first frame on."""
    n = 16 if len_snippet > 16 else int(len_snippet)
    return [int(start) + int(alternate) * i + 1 for i in range(n)]


# ---- device side -------------------------------------------------------------------------------------------------------

_TABLES = {}


def _dev_key(device: torch.device):
    return (device.type, device.index if device.index is not None else torch.cuda.current_device())


def device_table(device, in_size: int, out_size: int, filter: str):
    """``resample_table`` as two int32 tensors on ``device`` (cached), or None when the axis does not change."""
    if int(in_size) == int(out_size):
        return None
    key = ("rs", _dev_key(torch.device(device)), int(in_size), int(out_size), filter)
    t = _TABLES.get(key)
    if t is None:
        b, k = resample_table(in_size, out_size, filter)
        t = _TABLES[key] = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device))
    return t


def _lut(device, table: Optional[Tensor], norm_value, mean, std) -> Tensor:
    if table is not None:
        if table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] != 256:
            raise ValueError(f"video_input: a look-up table is float32 [C, 256], got {table.dtype} {tuple(table.shape)}")
        return table if table.is_cuda else table.to(device)
    if mean is None:
        key = ("target", _dev_key(torch.device(device)))
    else:
        key = ("norm", _dev_key(torch.device(device)), float(norm_value), tuple(float(v) for v in mean), tuple(float(v) for v in std))
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = (target_table() if mean is None else normalize_table(norm_value, mean, std)).to(device)
    return t


def _hw(size, what="size") -> Tuple[int, int]:
    try:
        h, w = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"video_input: {what} must be (h, w), got {size!r}") from None
    if h < 1 or w < 1:
        raise ValueError(f"video_input: {what} must be positive, got {size!r}")
    return h, w


def warm(device, src_size=None, size=None, pre_size=None, pre_filter: str = "bicubic", filter: str = "bilinear",
         norm_value=DATASET_NORM_VALUE, mean=DATASET_MEAN, std=DATASET_STD) -> None:
    """Build and upload now what the first call would: the look-up tables (normalisation and target) and, with ``src_size`` and
    ``size`` given as (h, w), the coefficient tables of ``transform_frames(frames of src_size, size, pre_size, ...)``."""
    device = torch.device(device)
    _lut(device, None, norm_value, mean, std)
    _lut(device, None, None, None, None)
    if src_size is not None and size is not None:
        cur = _hw(src_size, "src_size")
        for step, f in ((pre_size, pre_filter), (size, filter)):
            if step is None:
                continue
            nxt = _hw(step)
            device_table(device, cur[1], nxt[1], f)
            device_table(device, cur[0], nxt[0], f)
            cur = nxt


_FORMS = {None: ops.RESAMPLE_AUTO, True: ops.RESAMPLE_FUSED, False: ops.RESAMPLE_TWO_PASS}


def band_rows(src_size, size, channels: int = 3, filter: str = "bilinear") -> int:
    """Output rows per workgroup the fused form picks for this resize (0: a single pass, or no band fits in LDS and ``fused=None``
    takes the two-pass form)."""
    (H0, W0), (H1, W1) = _hw(src_size, "src_size"), _hw(size)
    return _lib.load().diffsal_resample_u8_band_rows(H0, W0, int(channels), H1, W1, _filter_id(filter))


def resize_u8(frames: Tensor, size, filter: str = "bilinear", fused: Optional[bool] = None, band: int = 0) -> Tensor:
    """One Pillow ``Image.resize((w, h), filter)`` of every frame: uint8 ``[N, H0, W0, C]`` (C = 1 or 3; ``[N, H0, W0]`` is taken as
    C = 1 and returned so) -> uint8 ``[N, h, w, C]`` with ``size = (h, w)``, bit-equal to Pillow.  ``fused=None`` picks the form
    (one launch with the intermediate image in LDS where a band fits and the source has at least twice the output's pixels,
    which is where it measured faster; else two passes through a workspace); ``True`` / ``False``
    force it; ``band`` forces the fused form's rows per workgroup.  Both forms give the same bits."""
    fid = _filter_id(filter)
    if fused not in _FORMS:
        raise ValueError(f"video_input: fused must be None, True or False, got {fused!r}")
    h, w = _hw(size)
    squeeze = isinstance(frames, Tensor) and frames.dim() == 3
    x = ops._u8_frames(frames[..., None] if squeeze else frames, "frames")
    dev = x.device
    out = ops.resample_u8(x, h, w, fid, device_table(dev, x.shape[2], w, filter), device_table(dev, x.shape[1], h, filter),
                          form=_FORMS[fused], band_rows=band)
    return out[..., 0] if squeeze else out


def transform_frames(frames: Tensor, size, pre_size=None, pre_filter: str = "bicubic", filter: str = "bilinear",
                     fused: Optional[bool] = None) -> Tensor:
    """The resize chain the reference applies to a decoded frame, uint8 in and out: ``pre_size`` with ``pre_filter`` first when
    given (the audio-visual datasets: ``pre_size=(240, 320)`` bicubic, the loader's ``img.resize((320, 240))``), then ``size`` with
    ``filter`` (``Scale`` / ``transforms.Resize``, bilinear).  DHF1K has no ``pre_size``.  The result may be kept per video: every
    clip of it is a ``gather_clips``."""
    x = frames
    if pre_size is not None:
        x = resize_u8(x, pre_size, pre_filter, fused)
    return resize_u8(x, size, filter, fused)


def _dst(dst, total: int, device) -> Optional[Tensor]:
    """The ``dst`` table of the grouped calls: a host sequence is range-checked and uploaded, a GPU tensor is used as it is."""
    if dst is None:
        return None
    if isinstance(dst, Tensor) and dst.is_cuda:
        if dst.dim() != 1 or dst.numel() != total or dst.is_floating_point() or dst.dtype == torch.bool:
            raise ValueError(f"video_input: dst must be {total} integers, got {dst.dtype} {tuple(dst.shape)}")
        return dst.to(torch.int32).contiguous()
    a = np.asarray(dst.numpy() if isinstance(dst, Tensor) else dst)
    if a.ndim != 1 or a.size != total or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"video_input: dst must be {total} integers, one per frame of the groups, got {a.dtype} {a.shape}")
    if (a < 0).any() or (a >= total).any():
        raise ValueError(f"video_input: dst entry outside 0 .. {total - 1}")
    return torch.from_numpy(a.astype(np.int32)).to(device)


def _group_list(groups, what: str = "groups"):
    if isinstance(groups, Tensor) or len(groups) == 0:
        raise ValueError(f"video_input: {what} must be a non-empty sequence of uint8 tensors [N, H, W, C]")
    return [ops._u8_frames(g, f"{what}[{i}]") for i, g in enumerate(groups)]


def resize_groups(groups, size, filter: str = "bilinear", fused: Optional[bool] = None, dst=None) -> Tensor:
    """``resize_u8`` of frames of several source sizes in one call: ``groups`` is a sequence of uint8 ``[N_g, H_g, W_g, C]`` (one C),
    the result uint8 ``[sum N_g, h, w, C]``.  Frame ``i`` of the concatenated groups lands at ``dst[i]`` (a permutation of
    ``range(sum N_g)``; None: at ``i``).  Group ``g``'s frames are bit-equal to ``resize_u8(groups[g], size, filter, fused)``, and
    each group takes the form that call would take.  The launches do not grow with the number of groups: at most three (fused
    bands, horizontal pass, vertical pass) per ``ops.RESAMPLE_MAX_GROUPS`` groups.  ``dst`` given on the host is range-checked here,
    before any launch; a GPU tensor is used as it is (the kernels clamp it)."""
    fid = _filter_id(filter)
    if fused not in _FORMS:
        raise ValueError(f"video_input: fused must be None, True or False, got {fused!r}")
    h, w = _hw(size)
    xs = _group_list(groups)
    dev = xs[0].device
    d = _dst(dst, sum(x.shape[0] for x in xs), dev)
    xt = [device_table(dev, x.shape[2], w, filter) for x in xs]
    yt = [device_table(dev, x.shape[1], h, filter) for x in xs]
    return ops.resample_u8_groups(xs, h, w, fid, xt, yt, form=_FORMS[fused], dst=d)


def transform_groups(groups, size, pre_size=None, pre_filter: str = "bicubic", filter: str = "bilinear", fused: Optional[bool] = None,
                     dst=None) -> Tensor:
    """``transform_frames`` of frames of several source sizes: the first resize of the chain is the grouped call; with ``pre_size``
    the second one has a single source size and is the existing call.  A single group in its own order goes through
    ``transform_frames``, the one-size route, which gives the same bytes."""
    xs = _group_list(groups)
    if len(xs) == 1 and dst is None:
        return transform_frames(xs[0], size, pre_size, pre_filter, filter, fused)
    if pre_size is not None:
        return resize_u8(resize_groups(xs, pre_size, pre_filter, fused, dst), size, filter, fused)
    return resize_groups(xs, size, filter, fused, dst)


def target_maps_groups(groups, size=SAMPLE_SIZE, filter: str = "bilinear", fused: Optional[bool] = None, dst=None) -> Tensor:
    """``target_maps`` of annotation maps of several sizes: ``groups`` a sequence of uint8 ``[N_g, H_g, W_g]`` (or ``[..., 1]``) ->
    float32 ``[sum N_g, 1, h, w]``, map ``i`` of the concatenated groups at ``dst[i]``."""
    if isinstance(groups, Tensor) or len(groups) == 0:
        raise ValueError("video_input: groups must be a non-empty sequence of uint8 maps [N, H, W]")
    xs = [g[..., None] if isinstance(g, Tensor) and g.dim() == 3 else g for g in groups]
    xs = _group_list(xs)
    if any(x.shape[3] != 1 for x in xs):
        raise ValueError(f"video_input: target_maps_groups takes single-channel maps, got {[tuple(x.shape) for x in xs]}")
    r = resize_u8(xs[0], size, filter, fused) if len(xs) == 1 and dst is None else resize_groups(xs, size, filter, fused, dst)
    N, h, w, _ = r.shape
    return ops.clip_gather_u8(r, None, N, 1, _lut(r.device, None, None, None, None)).view(N, 1, h, w)


def _indices(indices, n_frames: int, device) -> Tuple[Tensor, int, int]:
    if isinstance(indices, Tensor) and indices.is_cuda:
        if indices.dim() != 2 or indices.is_floating_point() or indices.dtype == torch.bool:
            raise ValueError(f"video_input: indices must be integers [B, T], got {indices.dtype} {tuple(indices.shape)}")
        return indices.to(torch.int32).contiguous(), indices.shape[0], indices.shape[1]
    a = np.asarray(indices.numpy() if isinstance(indices, Tensor) else indices)
    if a.ndim != 2 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"video_input: indices must be integers [B, T], got {a.dtype} {a.shape}")
    if (a < 0).any() or (a >= n_frames).any():
        raise ValueError(f"video_input: frame index outside 0 .. {n_frames - 1}")
    return torch.from_numpy(a.astype(np.int32)).to(device), a.shape[0], a.shape[1]


def gather_clips(resized: Tensor, indices, table: Optional[Tensor] = None, *, norm_value=DATASET_NORM_VALUE, mean=DATASET_MEAN,
                 std=DATASET_STD) -> Tensor:
    """``[B, 3, T, h, w]`` float32 from transformed frames uint8 ``[N, h, w, 3]``: clip ``b``, time ``t`` is frame
    ``indices[b][t]`` (0-based positions in ``resized``), each byte mapped through the look-up table of its channel: ``table``
    (float32 ``[3, 256]``) or ``normalize_table(norm_value, mean, std)``."""
    x = ops._u8_frames(resized, "resized")
    if x.shape[3] != 3:
        raise ValueError(f"video_input: gather_clips takes RGB frames [N, h, w, 3], got {tuple(x.shape)}")
    idx, B, T = _indices(indices, x.shape[0], x.device)
    return ops.clip_gather_u8(x, idx, B, T, _lut(x.device, table, norm_value, mean, std))


def clip_rgb(frames: Tensor, indices, size=SAMPLE_SIZE, pre_size=None, pre_filter: str = "bicubic", filter: str = "bilinear",
             table: Optional[Tensor] = None, *, norm_value=DATASET_NORM_VALUE, mean=DATASET_MEAN, std=DATASET_STD,
             fused: Optional[bool] = None) -> Tensor:
    """``data['rgb']`` of the reference for a batch of clips of one video: ``transform_frames`` then ``gather_clips``."""
    return gather_clips(transform_frames(frames, size, pre_size, pre_filter, filter, fused), indices, table, norm_value=norm_value,
                        mean=mean, std=std)


def target_maps(gt_u8: Tensor, size=SAMPLE_SIZE, filter: str = "bilinear", fused: Optional[bool] = None) -> Tensor:
    """``target['salmap']`` of the reference: annotation maps uint8 ``[N, H, W]`` (or ``[N, H, W, 1]``) -> float32 ``[N, 1, h, w]``,
    the bilinear ``transforms.Resize`` of the 'L' image and ``ToTensor``'s ``/ 255``."""
    x = gt_u8[..., None] if isinstance(gt_u8, Tensor) and gt_u8.dim() == 3 else gt_u8
    x = ops._u8_frames(x, "gt_u8")
    if x.shape[3] != 1:
        raise ValueError(f"video_input: target_maps takes single-channel maps, got {tuple(x.shape)}")
    r = resize_u8(x, size, filter, fused)
    N, h, w, _ = r.shape
    return ops.clip_gather_u8(r, None, N, 1, _lut(r.device, None, None, None, None)).view(N, 1, h, w)
