"""Benchmark-protocol saliency metrics on the device: AUC-Judd, AUC-Borji, shuffled AUC against the binary fixation map and
the benchmark forms of CC, NSS and SIM (R/metrics/metrics.py, which R/compute_metrics.py runs on PNG files in a pool of numpy
processes).  The predictions stay where the sampler left them: one kernel set (csrc/eval_metrics.hip, arithmetic in
include/diffsal.h "benchmark metrics") scores a batch per call, per image, in float64, without a host copy or a synchronisation.

Shapes and types: ``pred`` is ``[B, 1, H, W]`` or ``[B, H, W]`` (any floating type; computed from its fp32 values); fixation
maps are bool, uint8 (fixated iff non-zero) or floating (fixated iff ``> 0.5``, the reference's rule); ``gt`` is a floating map.
Every map must have ``pred``'s resolution: a shape mismatch raises here.  Quantising a prediction to 8 bits and resizing it to
the fixation map's resolution (the reference's PNG export and skimage ``resize``) is ``postprocess.protocol_metrics``, which
then calls this module.  There is no CPU path: CPU tensors raise.

Random locations of AUC-Borji / sAUC come either from an explicit ``rand_index`` table (``[B, n_rep, cap]`` int32 pixel
indices, -1 = unused: what parity with the reference uses) or from the device generator keyed by ``seed`` and a caller-supplied
non-negative ``image_ids`` entry per image (the dataset's frame index, not the position in the batch): an image's score then
does not depend on the batch it sits in.  The jitter of AUC-Judd comes from the same generator.

Definitions where the reference returns NaN or divides by zero: an image without fixations, with every pixel fixated or with a
flat map gets NaN in the fixation-based metrics (AUC-Judd, AUC-Borji, sAUC, NSS); its neighbours in the batch are unaffected.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from . import ops

Tensor = torch.Tensor
METRICS = ops.EVAL_ROWS


def _flat_pred(pred: Tensor, what: str = "pred"):
    if not isinstance(pred, Tensor) or not pred.is_cuda:
        raise RuntimeError(f"diff_sal_amd eval_metrics runs on the GPU only (no CPU fallback); {what} is on "
                           f"{getattr(pred, 'device', type(pred).__name__)}")
    if not pred.is_floating_point():
        raise ValueError(f"eval_metrics: {what} must be a floating map, got {pred.dtype}")
    if pred.dim() == 4 and pred.shape[1] == 1:
        pred = pred[:, 0]
    if pred.dim() != 3:
        raise ValueError(f"eval_metrics: {what} must be [B, 1, H, W] or [B, H, W], got {tuple(pred.shape)}")
    hw = tuple(pred.shape)
    return pred.reshape(hw[0], -1).float().contiguous(), hw


def _flat_map(t: Optional[Tensor], hw, what: str, binary: bool):
    if t is None:
        return None
    if not isinstance(t, Tensor) or not t.is_cuda:
        raise RuntimeError(f"diff_sal_amd eval_metrics runs on the GPU only (no CPU fallback); {what} is on "
                           f"{getattr(t, 'device', type(t).__name__)}")
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if tuple(t.shape) != tuple(hw):
        raise ValueError(f"eval_metrics: {what} {tuple(t.shape)} does not match pred {tuple(hw)} (resizing is out of scope "
                         "here: postprocess.protocol_metrics resizes the prediction first)")
    t = t.reshape(hw[0], -1)
    if not binary:
        if not t.is_floating_point():
            raise ValueError(f"eval_metrics: {what} must be a floating map, got {t.dtype}")
        return t.float().contiguous()
    if t.dtype == torch.bool or t.dtype == torch.uint8:
        return (t != 0).to(torch.uint8).contiguous()
    if t.is_floating_point():
        return (t > 0.5).to(torch.uint8).contiguous()
    raise ValueError(f"eval_metrics: {what} must be bool, uint8 or floating, got {t.dtype}")


def _rand(r: Optional[Tensor], B: int, n_rep: int, what: str):
    if r is None:
        return None
    if not isinstance(r, Tensor) or not r.is_cuda:
        raise RuntimeError(f"diff_sal_amd eval_metrics runs on the GPU only (no CPU fallback); {what} is not a GPU tensor")
    if r.dim() != 3 or r.shape[0] != B or r.shape[1] != n_rep or r.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"eval_metrics: {what} must be an integer tensor [B={B}, n_rep={n_rep}, cap], got {r.dtype} {tuple(r.shape)}")
    return r.to(torch.int32).contiguous()


def _key(image_ids, seed, device, B: int, why: str):
    if image_ids is None:
        raise ValueError(f"eval_metrics: {why} draws from the device generator and needs image_ids (one non-negative id per image)")
    ids_t, seed_t = ops.noise_key(image_ids, seed, device)
    if ids_t.numel() != B:
        raise ValueError(f"eval_metrics: {ids_t.numel()} image_ids for {B} images")
    return ids_t, seed_t


def benchmark_metrics(pred: Tensor, fix: Tensor, gt: Optional[Tensor] = None, other: Optional[Tensor] = None, *, jitter: bool = False,
                      n_rep: int = 100, step_size: float = 0.1, seed=0, image_ids=None, rand_index: Optional[Tensor] = None,
                      rand_index_shuffled: Optional[Tensor] = None, metrics=None) -> Dict[str, Tensor]:
    """Every metric the given inputs allow, as ``{name: [B] float64 device tensor}`` with the names of ``METRICS``: auc_judd,
    auc_borji and nss from ``fix``; cc and sim when ``gt`` is given; auc_shuffled when ``other`` (the union of other images'
    fixations) is given.  ``metrics`` restricts the set.  One call shares the min / max pass, the range-normalised map and the
    fixation lists between the terms.  ``jitter`` (reference default True, here False: it breaks the order of small values, as
    the reference's own docstring says) applies to AUC-Judd only."""
    p, hw = _flat_pred(pred)
    B = hw[0]
    f = _flat_map(fix, hw, "fix", True)
    g = _flat_map(gt, hw, "gt", False)
    o = _flat_map(other, hw, "other", True)
    want = set(METRICS if metrics is None else metrics)
    if not want <= set(METRICS):
        raise ValueError(f"eval_metrics: unknown metric(s) {sorted(want - set(METRICS))}; choose from {METRICS}")
    if f is None:
        want -= {"auc_judd", "auc_borji", "auc_shuffled", "nss"}
    if g is None:
        want -= {"cc", "sim"}
    if o is None:
        want -= {"auc_shuffled"}
    if not want:
        raise ValueError("eval_metrics: the inputs given allow none of the metrics asked for")
    n_rep = int(n_rep)
    rb = _rand(rand_index, B, n_rep, "rand_index") if "auc_borji" in want else None
    rs = _rand(rand_index_shuffled, B, n_rep, "rand_index_shuffled") if "auc_shuffled" in want else None
    if rb is not None and rs is not None and rb.shape[2] != rs.shape[2]:      # one cap per call: pad the narrower table with -1
        cap = max(rb.shape[2], rs.shape[2])
        rb = torch.nn.functional.pad(rb, (0, cap - rb.shape[2]), value=-1)
        rs = torch.nn.functional.pad(rs, (0, cap - rs.shape[2]), value=-1)
    need_gen = [why for why, on in (("jitter", jitter and "auc_judd" in want), ("auc_borji without rand_index", "auc_borji" in want and rb is None),
                                    ("auc_shuffled without rand_index_shuffled", "auc_shuffled" in want and rs is None)) if on]
    ids_t = seed_t = None
    if need_gen:
        ids_t, seed_t = _key(image_ids, seed, p.device, B, need_gen[0])
    bits = {"auc_judd": ops.EVAL_JUDD, "auc_borji": ops.EVAL_BORJI, "auc_shuffled": ops.EVAL_SAUC, "cc": ops.EVAL_CC,
            "nss": ops.EVAL_NSS, "sim": ops.EVAL_SIM}
    res: Dict[str, Tensor] = {}
    if jitter and "auc_judd" in want:      # the jittered map is Judd's alone: the other terms see the map as it is
        out = ops.eval_metrics(p, f, None, None, ops.EVAL_JUDD | ops.EVAL_JITTER, ids=ids_t, seed=seed_t)
        res["auc_judd"] = out[0]
        want = want - {"auc_judd"}
    if want:
        terms = 0
        for k in want:
            terms |= bits[k]
        out = ops.eval_metrics(p, f, g, o, terms, n_rep=n_rep, step=float(step_size), rand_borji=rb, rand_sauc=rs, ids=ids_t, seed=seed_t)
        for k in want:
            res[k] = out[METRICS.index(k)]
    return {k: res[k] for k in METRICS if k in res}


def auc_judd(pred: Tensor, fix: Tensor, *, jitter: bool = False, seed=0, image_ids=None) -> Tensor:
    """AUC_Judd (R/metrics/metrics.py:7-64) per image: [B] float64."""
    return benchmark_metrics(pred, fix, jitter=jitter, seed=seed, image_ids=image_ids, metrics=("auc_judd",))["auc_judd"]


def auc_borji(pred: Tensor, fix: Tensor, *, n_rep: int = 100, step_size: float = 0.1, seed=0, image_ids=None,
              rand_index: Optional[Tensor] = None) -> Tensor:
    """AUC_Borji (R/metrics/metrics.py:67-130) per image: [B] float64; locations from ``rand_index`` or the device generator."""
    return benchmark_metrics(pred, fix, n_rep=n_rep, step_size=step_size, seed=seed, image_ids=image_ids, rand_index=rand_index,
                             metrics=("auc_borji",))["auc_borji"]


def auc_shuffled(pred: Tensor, fix: Tensor, other: Tensor, *, n_rep: int = 100, step_size: float = 0.1, seed=0, image_ids=None,
                 rand_index: Optional[Tensor] = None) -> Tensor:
    """AUC_shuffled (R/metrics/metrics.py:133-175) per image: [B] float64; ``rand_index`` holds pixel indices taken from the
    fixated pixels of ``other``; without it every repetition takes min(n_fix, n_other) of them without replacement."""
    if other is None:
        raise ValueError("eval_metrics: auc_shuffled needs the other-image fixation map")
    return benchmark_metrics(pred, fix, other=other, n_rep=n_rep, step_size=step_size, seed=seed, image_ids=image_ids,
                             rand_index_shuffled=rand_index, metrics=("auc_shuffled",))["auc_shuffled"]


def cc(pred: Tensor, gt: Tensor) -> Tensor:
    """CC (R/metrics/metrics.py:203-224) per image: [B] float64."""
    p, hw = _flat_pred(pred)
    return ops.eval_metrics(p, None, _flat_map(gt, hw, "gt", False), None, ops.EVAL_CC)[3]


def nss(pred: Tensor, fix: Tensor) -> Tensor:
    """NSS (R/metrics/metrics.py:178-200) per image: [B] float64."""
    return benchmark_metrics(pred, fix, metrics=("nss",))["nss"]


def sim(pred: Tensor, gt: Tensor) -> Tensor:
    """SIM (R/metrics/metrics.py:227-252) per image: [B] float64."""
    p, hw = _flat_pred(pred)
    return ops.eval_metrics(p, None, _flat_map(gt, hw, "gt", False), None, ops.EVAL_SIM)[5]


class VideoMeter:
    """The aggregation of R/compute_metrics.py:105-109: the mean over a video's frames, then the mean over videos, rounded to four
    places.  ``update`` adds a batch of frames of ONE video (``metrics_dict``: name -> [B] tensor or scalar, e.g. the result of
    ``benchmark_metrics``); the per-video sums stay on the tensors' device and nothing is copied to the host before ``compute``.
    NaN propagates as in the reference (``nan_policy="propagate"``); ``"omit"`` leaves NaN frames out of a video's mean and videos
    without a valid frame out of the final mean."""

    def __init__(self, nan_policy: str = "propagate"):
        if nan_policy not in ("propagate", "omit"):
            raise ValueError(f"nan_policy must be 'propagate' or 'omit', got {nan_policy!r}")
        self.nan_policy = nan_policy
        self._sums: Dict[object, Dict[str, list]] = {}

    def update(self, video_key, metrics_dict) -> None:
        per = self._sums.setdefault(video_key, {})
        for name, v in metrics_dict.items():
            v = torch.as_tensor(v).detach().reshape(-1).to(torch.float64)
            if self.nan_policy == "omit":
                ok = ~torch.isnan(v)
                s, c = torch.where(ok, v, torch.zeros_like(v)).sum(), ok.sum().to(torch.float64)
            else:
                s, c = v.sum(), torch.tensor(float(v.numel()), dtype=torch.float64, device=v.device)
            if name in per:
                per[name][0] = per[name][0] + s
                per[name][1] = per[name][1] + c
            else:
                per[name] = [s, c]

    def compute(self) -> Dict[str, float]:
        """{name: mean over videos of the per-video frame means, rounded to 4 places}; the one host copy of the meter."""
        names = []
        for per in self._sums.values():
            names += [k for k in per if k not in names]
        out = {}
        for name in names:
            means = [per[name][0] / per[name][1] for per in self._sums.values() if name in per]      # 0 / 0 = NaN: no valid frame
            m = torch.stack(means)
            if self.nan_policy == "omit":
                m = m[~torch.isnan(m)]
            val = float(m.mean().item()) if m.numel() else float("nan")
            # np.around's arithmetic (scale, round half to even, unscale), not round(val, 4)'s correctly rounded decimal: the
            # two can differ in the last place when val * 1e4 lands on a half
            out[name] = round(val * 1e4) / 1e4 if math.isfinite(val) else val
        return out
