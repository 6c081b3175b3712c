"""The folder scorer: R/compute_metrics.py's walk of a folder of written predictions against a dataset folder, with the paths as
arguments instead of constants and every stage on the device.

The reference lists the sub-folders of ``pred_path`` as tasks; per task and video it pairs each prediction ``.png`` with the
annotation's ``maps`` and ``fixation`` files (three naming rules, ``pair_files``), reads the three files with ``plt.imread``,
computes AUC-Judd, CC, NSS and SIM per frame in a pool of 48 NumPy processes (resizing the prediction to the annotation's shape
with skimage wherever they differ), takes the mean over a video's frames, then over videos, rounds to four places and writes
``<pred_path>_metrics.csv``.  Here ``png.decode_files`` decodes the files, ``postprocess.from_uint8`` makes ``plt.imread``'s
floats, ``postprocess.protocol_metrics(..., quantize=False, anti_aliasing=True)`` resizes and scores a chunk of frames per call
and ``eval_metrics.VideoMeter`` takes the means: file bytes go up, one number per metric comes back, no pixel visits the host.

Differences from the reference, all deliberate:

* ``jitter`` is False, as everywhere in this package.  The reference's ``AUC_Judd`` defaults to ``jitter=True``, which draws from
  NumPy's global generator in 48 worker processes: its fourth decimal is not reproducible from run to run.  Pass ``jitter=True``
  with ``image_ids`` and ``seed`` for the device generator's jitter.
* a Hollywood-2 prediction whose index lies outside the annotation list is an error naming the file; the reference silently pairs
  it with the previous frame's annotation (or fails on the first frame).
* videos and tasks are walked in sorted order (the reference takes ``os.listdir``'s); a video's prediction folder without a
  ``.png`` is an error (the reference writes NaN for the whole task).
* the ``AUC_S `` column is 0.0 as the reference writes it, unless ``auc_borji=True`` asks for AUC-Borji there (what the
  reference's variable is called).

GPU only.  ``python -m diff_sal_amd.evaluate PRED_PATH DATA_TYPE --gt-root DIR`` is the command-line form.
"""
from __future__ import annotations

import csv as _csv
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

DATA_TYPES = ("dhf1k", "ucf", "holly")
DEFAULT_METRICS = ("auc_judd", "cc", "nss", "sim")
CSV_HEADER = ["Task", "AUC_J ", "AUC_S ", "CC ", "NSS ", "Sim"]      # the reference's, trailing blanks included
_CSV_COLUMNS = ("auc_judd", "auc_borji", "cc", "nss", "sim")


def _stems(folder: str) -> List[str]:
    """the reference's listing: the part in front of the first dot of every name that contains '.png', sorted as strings"""
    return sorted(n.split(".")[0] for n in os.listdir(folder) if ".png" in n)


def pair_files(pred_video_dir: str, gt_maps_dir: str, data_type: str, video) -> List[Tuple[str, str, str]]:
    """``[(prediction png, map png, fixation png)]`` of one video, in the order of the sorted prediction names
    (R/compute_metrics.py:65-103).  ``gt_maps_dir`` is the video's ``maps`` folder; the fixation file has the map's name in the
    ``fixation`` folder beside it.  Host code; only the two folders are listed, no file is opened.

    * ``dhf1k``: prediction ``<int>.png`` <-> map ``%04d.png`` of that integer;
    * ``ucf``: prediction ``<n>.png`` <-> map ``<name>_<clip>_%03d.png``, ``<name>-<clip>`` being the video's name split at its
      last hyphen;
    * ``holly``: prediction ``<k>.png`` <-> the k-th (from 1) of the sorted map names; a ``k`` outside the list is a ValueError."""
    if data_type not in DATA_TYPES:
        raise ValueError(f"evaluate: data_type must be one of {DATA_TYPES}, got {data_type!r}")
    maps_dir = gt_maps_dir.rstrip("/" + os.sep)
    fix_dir = os.path.join(os.path.dirname(maps_dir), "fixation")
    preds = _stems(pred_video_dir)
    names = []
    if data_type == "dhf1k":
        names = [(f"{int(s)}.png", f"{int(s):04d}.png") for s in preds]
    elif data_type == "ucf":
        parts = str(video).split("-")
        stem = "-".join(parts[:-1]) + "_" + parts[-1]
        names = [(f"{int(s.split('_')[-1])}.png", f"{stem}_{int(s):03d}.png") for s in preds]
    else:
        gts = _stems(maps_dir)
        for s in preds:
            k = int(s)
            if not 1 <= k <= len(gts):
                raise ValueError(f"evaluate: {os.path.join(pred_video_dir, s + '.png')} is prediction {k} of a video with "
                                 f"{len(gts)} annotated frames in {maps_dir}")
            names.append((s + ".png", gts[k - 1] + ".png"))
    return [(os.path.join(pred_video_dir, p), os.path.join(maps_dir, m), os.path.join(fix_dir, m)) for p, m in names]


def score_video(pairs: Sequence[Tuple[str, str, str]], *, batch: int = 64, **metric_kwargs) -> Dict[str, torch.Tensor]:
    """The per-frame metrics of one video's ``pairs`` (``pair_files``): ``{name: [n] float64 device tensor}``.  Per chunk of
    ``batch`` frames: the three files of every frame decoded on the device (``png.decode_files(..., "L")``), ``byte / 255`` as
    ``plt.imread`` gives it, a fixation where that exceeds 0.5, then ``postprocess.protocol_metrics(pred, fix, gt, quantize=False,
    anti_aliasing=True, metrics=("auc_judd", "cc", "nss", "sim"))``; ``metric_kwargs`` override or extend those keywords (``jitter``
    stays False unless given: see the module's docstring).  A video's predictions share one size and its annotations another."""
    from . import png
    from . import postprocess as pp

    pairs = list(pairs)
    if not pairs:
        raise ValueError("evaluate: score_video needs at least one frame")
    if int(batch) < 1:
        raise ValueError(f"evaluate: batch must be at least 1, got {batch}")
    kw = dict(quantize=False, anti_aliasing=True, metrics=DEFAULT_METRICS)
    kw.update(metric_kwargs)
    ids = kw.pop("image_ids", None)
    rows: Dict[str, list] = {}
    for lo in range(0, len(pairs), int(batch)):
        chunk = pairs[lo:lo + int(batch)]
        pred, gt, fix = (pp.from_uint8(png.decode_files([c[i] for c in chunk], "L")) for i in range(3))
        if ids is not None:
            kw["image_ids"] = ids[lo:lo + len(chunk)]
        for k, v in pp.protocol_metrics(pred, fix > 0.5, gt, **kw).items():
            rows.setdefault(k, []).append(v)
    return {k: torch.cat(v) for k, v in rows.items()}


def write_csv(path: str, results: Dict[str, Dict[str, float]]) -> None:
    """``results`` (``score_directory``'s) as the reference's table: its header, then per task the name, AUC-Judd, the ``AUC_S ``
    column (AUC-Borji where scored, else 0.0), CC, NSS, SIM."""
    with open(path, "w", newline="") as f:
        w = _csv.writer(f)
        w.writerow(CSV_HEADER)
        for task, r in results.items():
            w.writerow([task] + [r.get(k, 0.0 if k == "auc_borji" else float("nan")) for k in _CSV_COLUMNS])


def score_directory(pred_path: str, gt_root: str, data_type: str, videos: Optional[Sequence] = None, *, csv: bool = True,
                    auc_borji: bool = False, batch: int = 64, **metric_kwargs) -> Dict[str, Dict[str, float]]:
    """R/compute_metrics.py's ``main``: ``{task: {metric: mean}}`` for every sub-folder (task) of ``pred_path``, each holding one
    folder of prediction files per video.  The annotations of video ``v`` are ``<gt_root>/annotation/%04d/maps`` for ``dhf1k`` and
    ``<gt_root>/<v>/maps`` for ``ucf`` and ``holly``, with ``fixation`` beside ``maps``.  ``videos`` defaults to the reference's
    lists: 601 .. 700 for ``dhf1k``, the folders of ``gt_root`` otherwise; a video without a prediction folder is skipped.  Means
    go through ``VideoMeter``: over a video's frames, then over videos, rounded to four places.  ``csv=True`` writes
    ``pred_path + "_metrics.csv"`` (``write_csv``).  ``auc_borji=True`` also scores AUC-Borji (device generator, keyed by the
    frame's position in its video and ``seed``) and puts it where the reference writes 0.0.  ``jitter`` defaults to False: the
    reference's default jitter draws from NumPy's global generator and is not reproducible."""
    from . import eval_metrics as em

    if data_type not in DATA_TYPES:
        raise ValueError(f"evaluate: data_type must be one of {DATA_TYPES}, got {data_type!r}")
    pred_path = pred_path.rstrip("/" + os.sep)
    gt_path = os.path.join(gt_root, "annotation") if data_type == "dhf1k" else gt_root
    if videos is None:
        videos = range(601, 701) if data_type == "dhf1k" else sorted(os.listdir(gt_path))
    kw = dict(metric_kwargs)
    if auc_borji:
        kw["metrics"] = tuple(kw.get("metrics", DEFAULT_METRICS)) + ("auc_borji",)
    results: Dict[str, Dict[str, float]] = {}
    for task in sorted(t for t in os.listdir(pred_path) if os.path.isdir(os.path.join(pred_path, t))):
        meter = em.VideoMeter()
        for vid in videos:
            pred_dir = os.path.join(pred_path, task, str(vid))
            if not os.path.isdir(pred_dir):
                continue
            maps_dir = os.path.join(gt_path, f"{int(vid):04d}" if data_type == "dhf1k" else str(vid), "maps")
            pairs = pair_files(pred_dir, maps_dir, data_type, vid)
            if not pairs:
                raise ValueError(f"evaluate: {pred_dir} holds no .png prediction")
            if auc_borji and "image_ids" not in metric_kwargs:
                kw["image_ids"] = list(range(len(pairs)))
            meter.update(vid, score_video(pairs, batch=batch, **kw))
        results[task] = meter.compute()
    if csv:
        write_csv(pred_path + "_metrics.csv", results)
    return results


def main(argv=None) -> None:
    import argparse

    ap = argparse.ArgumentParser(prog="python -m diff_sal_amd.evaluate", description="Score a folder of written predictions "
                                 "(<pred_path>/<task>/<video>/<frame>.png) against a dataset folder; writes <pred_path>_metrics.csv")
    ap.add_argument("prediction_path")
    ap.add_argument("data_type", choices=DATA_TYPES)
    ap.add_argument("--gt-root", required=True, help="the dataset folder (dhf1k: the one that holds annotation/)")
    ap.add_argument("--auc-borji", action="store_true", help="score AUC-Borji into the AUC_S column (the reference writes 0.0)")
    ap.add_argument("--batch", type=int, default=64, help="frames per device call")
    args = ap.parse_args(argv)
    for task, r in score_directory(args.prediction_path, args.gt_root, args.data_type, auc_borji=args.auc_borji, batch=args.batch).items():
        print(task, r)


if __name__ == "__main__":
    main()
