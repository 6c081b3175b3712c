"""From a dataset folder to trained weights: the reference trainer's ``train()`` and ``train_av_data()`` loops
(R/diffusion_trainer.py:139-432) over its ``mode="train"`` datasets, around the step this package already has
(``DiffusionTrainStep``: forward, hand-written backward, gradient exchange, clip, Adam, all on the device).

    listing --epoch_order--> index lists --load_batches--> img [B, 3, 16, h, w], salmap [B, 1, h, w], audio [B, 1, 9, h/2, w/2]
      --trainer.step(salmap, cond, sample_ids=...)--> ... --ckpt_<epoch>.pth, train.log, val.log, best.pth

* ``list_train_clips`` / ``list_av_train_clips`` are the training listings (host code: folders are listed, no file is opened);
* ``drop_empty_maps`` removes the clips whose target map is all zero;
* ``epoch_order`` is the shuffled, sharded, batched order of one epoch, a pure function of its arguments;
* ``load_batches`` is the front end for one or several steps' batches in one go.  A shuffled batch holds clips of different
  videos, and outside DHF1K every video has its own resolution: the files are decoded per geometry (``png`` / ``jpeg``
  ``.decode_groups``) and every frame of the load, of any source size, is resized by one grouped call
  (``video_input.transform_groups``, ``target_maps_groups``) whose launch count does not depend on the number of geometries;
* ``fit_directory`` is ``train()`` for DHF1K, UCF-Sports and Hollywood-2, ``fit_av`` is the loop of ``train_av_data()`` for one
  split of the audio-visual sets.

Differences from the reference's loops, all deliberate:

* ``epoch_order`` reshuffles every epoch.  The reference never calls ``DistributedSampler.set_epoch``, so under DDP it repeats
  the order of epoch 0 in every epoch; with one process it shuffles through torch's global generator.  Here the order is
  ``DistributedSampler``'s for ``seed`` and the epoch set, for any number of ranks, so a resumed run sees the order the
  uninterrupted one saw;
* the audio-visual dataset of the reference replaces a clip whose target map is all zero by a random other item at load time
  (R/datasets/saliency_db.py:390-392: ``np.random.randint(0, index - 1)``, which fails for the first two items).  ``fit_av``
  calls ``drop_empty_maps`` on the listing instead, once, by default: such clips are never drawn, and they are reported;
* videos are walked in sorted order where the reference takes ``os.listdir``'s, and the UCF name is taken apart at its last
  hyphen (see ``predict.list_clips``);
* the loss meters live on the device.  The reference's ``AverageMeterList`` reads every step's five values to the host
  (``round(v.item(), 3)``, R/util/utils.py:47-50); here every step adds ``round(v * 1000) / 1000`` (float64, on the device) to a
  device sum, and the sums are read only every ``log_freq`` steps and at the epoch's end: no host synchronisation inside a step.
  The two roundings differ only for a value whose float64 image lies within an ulp of a half-thousandth;
* a resumed run continues the learning-rate schedule where the checkpoint left it.  The reference builds a fresh
  ``MultiStepLR`` on resuming, which counts its milestones from the resumed epoch;
* the three-split loop of ``train_av_data`` and the model dump ``training_model.txt`` are left to the caller.

GPU only: a CPU model raises.
"""
from __future__ import annotations

import contextlib
import csv
import math
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _image_files, predict, video_input
from .predict import AVClip, Clip

Tensor = torch.Tensor

DHF1K_TRAIN = range(1, 601)                        # video_names[:600] of the complete set, R/datasets/dhf1k_data.py:29
TRAIN_HEADER = ("epoch", "total_step", "loss", "main", "cc", "sim", "nss", "lr")      # R/diffusion_trainer.py:172-175, 317-320
VAL_HEADER = ("epoch", "total_step", "loss", "main", "cc", "sim", "nss")              # R/diffusion_trainer.py:176-179, 321-324
LOSS_NAMES = predict.LOSS_NAMES
# Chosen from the table in DESIGN.md ("Training driver"), by its rule: the pair with the lowest data time per step that the step
# does not hide.  Measured at batch 4 on one MI355X with 16 host CPUs, ms per step at steps_per_load 1 / 4 / 8: JPEG frames of eight
# geometries, device 99.3 / 52.5 / 30.9, host 28.4 / 17.0 / 12.7; 360 x 640 PNG frames, device 237.5 / 72.4 / 37.6, host 34.9 / 44.0 /
# 39.3; the full-size step takes 63.3 ms.  ("host", 8) has the lowest sum over the two trees (52.0 ms; ("host", 4) 61.0, ("host", 1)
# 63.3, ("device", 8) 68.5), and the host decode is the part the prefetch thread runs under the current steps, while the device
# decode runs in the training stream and adds to every step.
DEFAULT_DECODE = "host"
DEFAULT_STEPS_PER_LOAD = 8


# ---- listings (host) ----------------------------------------------------------------------------------------------------

def skip_window(len_snippet: int) -> int:
    """The stride of the training starts (R/datasets/meta_data.py:37-41): 16 for a ``len_snippet`` above 16, else ``len_snippet``."""
    return 16 if int(len_snippet) > 16 else int(len_snippet)


def list_train_clips(data_type: str, root: str, *, len_snippet: int = 32, alternate: int = 1,
                     videos: Optional[Sequence] = None) -> List[Clip]:
    """The reference's ``mode="train"`` listing of a visual set under ``root``, in its order: per video, every start in turn.

    Quirks of the reference that are kept:

    * the starts are ``range(0, n - alternate * len_snippet, skip_window)`` with ``n`` the number of entries of the frame folder
      and ``skip_window = 16 if len_snippet > 16 else len_snippet`` (R/datasets/meta_data.py:37-41); a video of exactly
      ``alternate * len_snippet`` frames gives no clip;
    * a clip holds 16 frames whatever a ``len_snippet`` above 16 says (R/datasets/dhf1k_data.py:70-74);
    * ``dhf1k`` (R/datasets/dhf1k_data.py:28-29, 33-39): the first 600 videos, folders named 1 .. 600 under ``<root>/frames``; files
      ``'%d.png'`` of ``start + alternate * i + 1``; the map is ``<root>/maps/<video>/%04d.png`` of element 8 of those numbers;
    * ``ucf`` (R/datasets/ucf_dataset.py:25-31) and ``holly`` (R/datasets/holly2wood_dataset.py:24-32): the videos under
      ``<root>/training``, frames in ``<video>/images``, maps in ``<video>/maps``.  Train mode has no short-video skip and no extra
      last clip: a video shorter than ``alternate * len_snippet`` is not skipped, its range of starts is simply empty;
    * ``ucf`` files are ``<name>_<clip>_%03d.png`` of the 1-based numbers; ``holly`` uses the 0-based positions
      ``start + alternate * i`` in the sorted listing of ``images``, for the frames and for the map.

    Differences, deliberate, as in ``predict.list_clips``: ``ucf`` / ``holly`` videos come in sorted order (the reference:
    ``os.listdir``'s); the ``ucf`` video name is taken apart at its last hyphen (the reference's ``str.strip`` removes characters,
    not a suffix); ``dhf1k`` takes the folders whose integer name is 1 .. 600, in integer order (the reference: positions 0 .. 599
    of the integer-sorted listing, the same on the complete set); ``videos``, when given, replaces the video list.

    No file is opened; folders are listed."""
    if data_type not in predict.DATA_TYPES:
        raise ValueError(f"train: data_type must be one of {predict.DATA_TYPES}, got {data_type!r}")
    len_snippet, alternate = int(len_snippet), int(alternate)
    if len_snippet < 1 or alternate < 1:
        raise ValueError(f"train: len_snippet and alternate must be at least 1, got {len_snippet}, {alternate}")
    root = os.fspath(root)
    stride = skip_window(len_snippet)
    clips: List[Clip] = []
    if data_type == "dhf1k":
        img_path, ann_path = os.path.join(root, "frames"), os.path.join(root, "maps")
        if videos is None:
            videos = sorted((v for v in os.listdir(img_path) if v.isdigit() and int(v) in DHF1K_TRAIN), key=int)
        for v in (str(v) for v in videos):
            n = len(os.listdir(os.path.join(img_path, v)))
            for start in range(0, n - alternate * len_snippet, stride):
                numbers = video_input.dhf1k_indices(start, alternate, len_snippet)
                gt = numbers[len(numbers) // 2]
                clips.append(Clip(v, tuple(os.path.join(img_path, v, "%d.png" % i) for i in numbers), gt,
                                  os.path.join(ann_path, v, "%04d.png" % gt)))
        return clips
    base = os.path.join(root, "training")
    if videos is None:
        videos = sorted(os.listdir(base))
    for v in (str(v) for v in videos):
        images, maps = os.path.join(base, v, "images"), os.path.join(base, v, "maps")
        names = sorted(os.listdir(images))
        n = len(names)
        if data_type == "ucf":
            name, sep, number = v.rpartition("-")
            if not sep:
                raise ValueError(f"train: ucf video {v!r} has no hyphen to take its name apart at")
        for start in range(0, n - alternate * len_snippet, stride):
            numbers = video_input.dhf1k_indices(start, alternate, len_snippet)
            if data_type == "ucf":
                gt = numbers[len(numbers) // 2]
                files = ["{}_{}_{:03d}.png".format(name, number, i) for i in numbers]
                gt_name = "{}_{}_{:03d}.png".format(name, number, gt)
            else:
                positions = [i - 1 for i in numbers]
                gt = positions[len(positions) // 2]
                files = [names[i] for i in positions]      # start + 16 alternate <= n - 1 for a len_snippet of 16 or more
                gt_name = names[gt]
            clips.append(Clip(v, tuple(os.path.join(images, f) for f in files), gt, os.path.join(maps, gt_name)))
    return clips


def list_av_train_clips(video_root: str, fold_list: str, salmap_root: str, audio_root: str, *, sample_duration: int = predict.CLIP_FRAMES,
                        step_duration: int = 90) -> List[AVClip]:
    """The non-exhaustive listing of ``saliency_db_spec`` (R/datasets/saliency_db.py:173-252, 269-276), the one its training loader
    uses: videos are skipped as in ``predict.list_av_clips``; with ``step = max(1, step_duration - sample_duration)`` every
    ``j in range(1, nframes, step)`` gives one clip whose window is ``range(j, min(nframes + 1, j + step_duration))``, cut to
    ``sample_duration`` frames around its middle by ``video_input.center_crop_indices`` (a shorter window is walked again from its
    head) and labelled by ``video_input.median_index`` of the result.  Files: ``img_%05d.jpg``, ``maps/eyeMap_%05d.jpg``."""
    video_root = os.fspath(video_root).rstrip("/" + os.sep)
    dataset = os.path.basename(video_root)
    sample_duration, step_duration = int(sample_duration), int(step_duration)
    step = max(1, step_duration - sample_duration)
    clips: List[AVClip] = []
    for name, n_frames, fps in predict.read_fold_list(fold_list):
        video_path = os.path.join(video_root, name)
        annot_path = os.path.join(salmap_root, name, "maps")
        wav_path = os.path.join(audio_root, name, name + ".wav")
        if not os.path.exists(video_path) or not os.path.exists(annot_path) or n_frames <= 1 or not os.path.exists(wav_path):
            continue
        for j in range(1, n_frames, step):
            idx = video_input.center_crop_indices(range(j, min(n_frames + 1, j + step_duration)), sample_duration)
            med = video_input.median_index(idx)
            clips.append(AVClip(name, f"{dataset}/{name}", tuple(idx), tuple(os.path.join(video_path, "img_{:05d}.jpg".format(i)) for i in idx),
                                med, os.path.join(annot_path, "eyeMap_{:05d}.jpg".format(med)), wav_path, n_frames, fps))
    return clips


def epoch_order(n: int, epoch: int, seed: int, rank: int = 0, world: int = 1, batch: int = 1) -> List[List[int]]:
    """The batches of rank ``rank`` in epoch ``epoch`` as lists of indices into a listing of ``n`` items: what
    ``DataLoader(dataset, batch_size=batch, drop_last=True, sampler=DistributedSampler(dataset, world, rank, shuffle=True,
    seed=seed))`` yields after ``sampler.set_epoch(epoch)`` (R/datasets/prepare_data.py:8-24 sets the loader up so):

    * ``torch.randperm(n, generator=torch.Generator().manual_seed(seed + epoch))`` on the CPU;
    * padded to a multiple of ``world`` by walking the permutation again from its head, then every ``world``-th index from
      ``rank`` on;
    * cut into batches of ``batch``, the incomplete last one dropped.

    A pure function of its arguments.  The reference never calls ``set_epoch`` and so repeats epoch 0's order; this function is
    called with the running epoch (see the module's docstring)."""
    n, epoch, seed, rank, world, batch = int(n), int(epoch), int(seed), int(rank), int(world), int(batch)
    if n < 1 or batch < 1 or world < 1 or not 0 <= rank < world or epoch < 0:
        raise ValueError(f"train: epoch_order(n={n}, epoch={epoch}, rank={rank}, world={world}, batch={batch})")
    g = torch.Generator()
    g.manual_seed(seed + epoch)
    indices = torch.randperm(n, generator=g).tolist()
    per_rank = math.ceil(n / world)
    pad = per_rank * world - n
    if pad <= n:
        indices += indices[:pad]
    else:
        indices += (indices * math.ceil(pad / n))[:pad]
    own = indices[rank:per_rank * world:world]
    return [own[i:i + batch] for i in range(0, per_rank - batch + 1, batch)]


# ---- front end ------------------------------------------------------------------------------------------------------------

def _codec(path: str):
    from . import jpeg, png

    ext = os.path.splitext(path)[1].lower()
    if ext == ".png":
        return png
    if ext in (".jpg", ".jpeg"):
        return jpeg
    raise ValueError(f"train: {path}: frame and map files are .png or .jpg")


def _pil_read(path_mode) -> np.ndarray:
    from PIL import Image

    path, mode = path_mode
    with Image.open(path) as im:
        return np.asarray(im.convert(mode))


def _read_images(paths: Sequence[str], mode: str, decode: str, threads: int) -> list:
    """what travels to the device for the files at ``paths``: their bytes (``decode="device"``) or, decoded with Pillow in the
    reader threads, their pixels as uint8 arrays (``decode="host"``)"""
    if decode == "device":
        return _image_files.read_files(paths, threads)
    n = min(int(threads), _image_files.MAX_READ_THREADS, len(paths))
    jobs = [(p, mode) for p in paths]
    if n <= 1:
        return [_pil_read(j) for j in jobs]
    with ThreadPoolExecutor(max_workers=n) as pool:
        return list(pool.map(_pil_read, jobs))


def _to_groups(paths: Sequence[str], items: list, mode: str, decode: str, device) -> Tuple[list, List[int]]:
    """``(groups, dst)``: the items (``_read_images``) as one uint8 tensor per geometry on ``device``, and the ``dst`` table of the
    grouped resize, which puts the frame at position ``p`` of the concatenated groups back at its position in ``paths``"""
    groups: list = []
    where: List[Tuple[int, int]] = [(0, 0)] * len(paths)
    if decode == "device":
        by_codec: Dict[object, List[int]] = {}
        for i, p in enumerate(paths):
            by_codec.setdefault(_codec(p), []).append(i)
        for codec, at in by_codec.items():
            g, w = codec.decode_groups([items[i] for i in at], mode, device)
            for i, (gi, k) in zip(at, w):
                where[i] = (len(groups) + gi, k)
            groups += g
    else:
        index: Dict[tuple, int] = {}
        members: List[List[int]] = []
        for i, a in enumerate(items):
            gi = index.setdefault(a.shape, len(index))
            if gi == len(members):
                members.append([])
            where[i] = (gi, len(members[gi]))
            members[gi].append(i)
        groups = [torch.from_numpy(np.stack([items[i] for i in m])).to(device) for m in members]
    first = np.concatenate([[0], np.cumsum([g.shape[0] for g in groups])])
    dst = [0] * len(paths)
    for i, (gi, k) in enumerate(where):
        dst[int(first[gi]) + k] = i
    return groups, dst


def _unique(items: Sequence) -> Tuple[list, Dict]:
    where: Dict = {}
    for it in items:
        where.setdefault(it, len(where))
    return list(where), where


@dataclass
class _HostLoad:
    """what the host threads prepare for one load: the listing positions of every step, the files each read once, the audio"""
    steps: List[List[int]]
    frame_files: List[str]
    frame_items: list
    rows: List[List[int]]              # per clip of the load, its frames as positions in frame_files
    map_files: List[str]
    map_items: list
    map_at: List[int]                  # per clip of the load, its map as a position in map_files
    waves: Optional[list] = None       # per distinct .wav of the load, (samples int16, rate)
    wave_at: Optional[List[int]] = None


def _host_load(clips: Sequence, steps: Sequence[Sequence[int]], decode: str, threads: int, audio: bool) -> _HostLoad:
    steps = [[int(i) for i in s] for s in steps]
    flat = [clips[i] for s in steps for i in s]
    frame_files, rows = predict._positions(flat)
    map_files, map_where = _unique([c.gt_file for c in flat])
    load = _HostLoad(steps, frame_files, _read_images(frame_files, "RGB", decode, threads), rows, map_files,
                     _read_images(map_files, "L", decode, threads), [map_where[c.gt_file] for c in flat])
    if audio:
        wav_files, wav_where = _unique([c.wav_file for c in flat])
        load.waves = [predict.read_wav(f) for f in wav_files]
        load.wave_at = [wav_where[c.wav_file] for c in flat]
    return load


def _device_load(clips: Sequence, load: _HostLoad, size, device, decode: str, norm, audio_kw: Optional[dict]) -> List[dict]:
    flat = [clips[i] for s in load.steps for i in s]
    av = isinstance(flat[0], AVClip)
    groups, dst = _to_groups(load.frame_files, load.frame_items, "RGB", decode, device)
    resized = video_input.transform_groups(groups, size, pre_size=predict.AV_PRE_SIZE if av else None, pre_filter="bicubic", dst=dst)
    del groups
    mgroups, mdst = _to_groups(load.map_files, load.map_items, "L", decode, device)
    targets = video_input.target_maps_groups(mgroups, size, dst=mdst)
    del mgroups
    audio = None
    if load.waves is not None:
        audio = _clip_audio(flat, load, size, device, audio_kw or {})
    out, lo = [], 0
    for s in load.steps:
        hi = lo + len(s)
        batch = {"img": video_input.gather_clips(resized, load.rows[lo:hi], **norm),
                 "salmap": targets[torch.as_tensor(load.map_at[lo:hi], device=device)], "sample_ids": list(s)}
        if audio is not None:
            batch["audio"] = audio[lo:hi]
        out.append(batch)
        lo = hi
    return out


def _clip_audio(flat: Sequence[AVClip], load: _HostLoad, size, device, kw: dict) -> Tensor:
    """``data['audio']`` of every clip of the load: the distinct ``.wav`` files as one int16 ``[V, Lmax]`` tensor, one
    ``audio_input.clip_audio`` call per distinct sample rate (usually one)"""
    from . import audio_input

    window = audio_input.DEFAULT_WINDOW if kw.get("window") is None else int(kw["window"])
    resample = kw.get("resample", "kaiser_best")
    lengths = [w[0].shape[0] for w in load.waves]
    host = np.zeros((len(load.waves), max(max(lengths), 1)), dtype=np.int16)
    for v, (samples, _) in enumerate(load.waves):
        host[v, :samples.shape[0]] = samples
    wav = torch.from_numpy(host).to(device)
    tables = {}
    starts, ends = [], []
    for c, v in zip(flat, load.wave_at):
        key = (v, c.n_frames, c.fps)
        if key not in tables:
            tables[key] = audio_input.excerpt_table(c.n_frames, c.fps, load.waves[v][1], lengths[v])
        s, e = tables[key]
        starts.append(int(s[c.frame_indices[0]]))
        ends.append(int(e[c.frame_indices[-1]]))
    h, w = size
    out = torch.empty((len(flat), 1, audio_input.NUM_EXAMPLES, h // 2, w // 2), device=device, dtype=torch.float32)
    by_rate: Dict[int, List[int]] = {}
    for b, v in enumerate(load.wave_at):
        by_rate.setdefault(int(load.waves[v][1]), []).append(b)
    for rate, at in by_rate.items():
        rate_kw = {} if rate == audio_input.SAMPLE_RATE else dict(sample_rate=rate, resample=resample)
        a = audio_input.clip_audio(wav, [starts[b] for b in at], [ends[b] for b in at], size=(h // 2, w // 2), window=window,
                                   wav_len=lengths, video=[load.wave_at[b] for b in at], **rate_kw)
        if len(by_rate) == 1:
            return a
        out[torch.as_tensor(at, device=device)] = a
    return out


def _norm(clips: Sequence, norm_value, mean, std) -> dict:
    """the normalisation of the set's loader: R/datasets/meta_data.py:27-31 for the visual sets, R/cfgs/dataset.json for the others"""
    av = isinstance(clips[0], AVClip)
    return dict(norm_value=(video_input.DATASET_NORM_VALUE if av else 255) if norm_value is None else norm_value,
                mean=(video_input.DATASET_MEAN if av else video_input.IMAGENET_MEAN) if mean is None else mean,
                std=(video_input.DATASET_STD if av else video_input.IMAGENET_STD) if std is None else std)


def _check_decode(decode: str, steps_per_load) -> None:
    if decode not in ("device", "host"):
        raise ValueError(f"train: decode must be 'device' or 'host', got {decode!r}")
    if steps_per_load is not None and int(steps_per_load) < 1:
        raise ValueError(f"train: steps_per_load must be at least 1, got {steps_per_load}")


def load_batches(clips: Sequence, index_lists: Sequence[Sequence[int]], size=video_input.SAMPLE_SIZE, *, device=None,
                 decode: str = DEFAULT_DECODE, steps_per_load: Optional[int] = None, threads: int = 16, audio: Optional[bool] = None,
                 norm_value=None, mean=None, std=None, window: Optional[int] = None, resample="kaiser_best") -> List[dict]:
    """The training inputs of the steps ``index_lists`` (lists of positions in ``clips``, as ``epoch_order`` gives them): per step a
    dictionary with ``img [B, 3, 16, h, w]``, ``salmap [B, 1, h, w]``, for audio-visual clips ``audio [B, 1, 9, h/2, w/2]``, and
    ``sample_ids``, the clips' positions in the listing.

    ``steps_per_load`` steps share one front-end call (None: all of them).  Per call: every frame file any of its clips uses is
    read once (``threads`` host threads, at most 16), decoded in one call per distinct geometry (``decode_groups``) and resized
    with all the others in one grouped call (``video_input.transform_groups``; ``pre_size=(240, 320)`` bicubic first for the
    audio-visual sets); the maps likewise (``target_maps_groups``); every step's clips are then a ``gather_clips``.  One file is
    one wave's serial work whatever the count, so a larger load keeps more of the device busy; it also holds more geometries, which
    the grouped resize does not pay for in launches.  The ``.wav`` files are read on the host and the clips' audio is
    ``audio_input.clip_audio`` in its ``[V, Lmax]`` form (``audio=False`` leaves it out; default: audio-visual clips get it).

    ``decode="device"``: only file bytes travel.  ``decode="host"``: the files are decoded with Pillow in the reader threads and
    uint8 frames travel; everything after the decode is identical, and so are the tensors.  The normalisation defaults to the
    set's loader's (``norm_value`` / ``mean`` / ``std`` override it)."""
    _check_decode(decode, steps_per_load)
    clips = list(clips)
    lists = [list(s) for s in index_lists]
    if not clips or not lists or any(len(s) == 0 for s in lists):
        raise ValueError("train: load_batches takes a non-empty listing and non-empty index lists")
    if any(not 0 <= int(i) < len(clips) for s in lists for i in s):
        raise ValueError(f"train: an index outside the listing of {len(clips)} clips")
    size = video_input._hw(size)
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError(f"diff_sal_amd train runs on the GPU only (no CPU fallback); load_batches got device {dev}")
    want_audio = isinstance(clips[0], AVClip) if audio is None else bool(audio)
    norm = _norm(clips, norm_value, mean, std)
    per = len(lists) if steps_per_load is None else int(steps_per_load)
    out: List[dict] = []
    for lo in range(0, len(lists), per):
        load = _host_load(clips, lists[lo:lo + per], decode, threads, want_audio)
        out += _device_load(clips, load, size, dev, decode, norm, dict(window=window, resample=resample))
    return out


def drop_empty_maps(clips: Sequence, size=video_input.SAMPLE_SIZE, *, device=None, decode: str = DEFAULT_DECODE, threads: int = 16,
                    files_per_call: int = 1024) -> Tuple[list, list]:
    """``(kept, removed)``: the clips whose target map -- ``target_maps`` of the listed map file at ``size``, what the reference
    tests with ``target['salmap'].max() == 0`` (R/datasets/saliency_db.py:389-390) -- is not all zero, and those where it is, both
    in list order.  Every distinct map file is decoded once, ``files_per_call`` files per grouped call, and one flag per file is
    read back per call.  The reference replaces such a clip by a random other item each time it is drawn; removing it from the
    listing once is the deliberate difference (see the module's docstring)."""
    _check_decode(decode, None)
    clips = list(clips)
    size = video_input._hw(size)
    dev = torch.device("cuda" if device is None else device)
    files, where = _unique([c.gt_file for c in clips])
    blank: List[bool] = []
    for lo in range(0, len(files), int(files_per_call)):
        part = files[lo:lo + int(files_per_call)]
        groups, dst = _to_groups(part, _read_images(part, "L", decode, threads), "L", decode, dev)
        targets = video_input.target_maps_groups(groups, size, dst=dst)
        blank += (targets.flatten(1).amax(1) == 0).cpu().tolist()
    kept = [c for c in clips if not blank[where[c.gt_file]]]
    removed = [c for c in clips if blank[where[c.gt_file]]]
    return kept, removed


# ---- the loop -------------------------------------------------------------------------------------------------------------

@dataclass
class FitReport:
    """What a driver did: the ``epochs`` it ran (1-based numbers), the global ``step`` it ended at, the ``train_rows`` / ``val_rows``
    it logged (dictionaries with the logs' columns), the ``checkpoints`` written, the epochs at which ``best.pth`` was written
    and the clips ``removed`` by ``drop_empty_maps``."""
    epochs: List[int] = field(default_factory=list)
    step: int = 0
    train_rows: List[dict] = field(default_factory=list)
    val_rows: List[dict] = field(default_factory=list)
    checkpoints: List[str] = field(default_factory=list)
    best_epochs: List[int] = field(default_factory=list)
    removed: list = field(default_factory=list)


class Logger:
    """The reference's ``Logger`` (R/util/utils.py:74-95): a tab-separated file opened for appending, the header written at once,
    a column missing from a row written as 0.0."""

    def __init__(self, path: str, header: Sequence[str]):
        self.header = list(header)
        self.file = open(path, "a+", newline="")
        self.writer = csv.writer(self.file, delimiter="\t")
        self.writer.writerow(self.header)
        self.file.flush()

    def log(self, values: dict) -> None:
        self.writer.writerow([values.get(col, 0.0) for col in self.header])
        self.file.flush()

    def close(self) -> None:
        self.file.close()


class DeviceMeters:
    """``AverageMeterList`` (R/util/utils.py:37-53) without its host reads: ``update`` adds every value, rounded to 3 places, to a
    float64 sum on the device; ``means`` is the one read-back."""

    def __init__(self, device):
        self.sums = torch.zeros(len(LOSS_NAMES), dtype=torch.float64, device=device)
        self.count = 0

    def update(self, losses: dict) -> None:
        v = torch.stack([losses[k].detach().double().reshape(()) if torch.is_tensor(losses[k]) else self.sums.new_full((), float(losses[k]))
                         for k in LOSS_NAMES])
        self.sums += torch.round(v * 1000.0) / 1000.0
        self.count += 1

    def means(self) -> Dict[str, float]:
        s = self.sums.cpu().tolist()
        return {k: (s[i] / self.count if self.count else float("nan")) for i, k in enumerate(LOSS_NAMES)}


def train_row(epoch: int, step: int, means: Dict[str, float], lr: float) -> dict:
    """A row of ``train.log`` as ``print_train_info`` writes it (R/diffusion_trainer.py:977-988): ``epoch`` is the 1-based number."""
    return {"epoch": epoch, "total_step": step, "loss": round(means["total"], 3), "main": round(means["main"], 3),
            "cc": round(means["cc"], 3), "sim": round(means["sim"], 3), "nss": round(means["nss"], 3), "lr": lr}


def val_row(epoch: int, step: int, means: Dict[str, float]) -> dict:
    """A row of ``val.log`` as ``print_val_info`` writes it (R/diffusion_trainer.py:1010-1020)."""
    row = train_row(epoch, step, means, 0.0)
    del row["lr"]
    return row


class BestKeeper:
    """The reference's rule for ``best.pth`` (R/diffusion_trainer.py:196, 276-280, 339, 426-428), restated as it is:
    ``min_loss`` starts at 0.0 and a checkpoint is the best when ``cur_val_loss > min_loss``, which then becomes ``min_loss``.
    ``cur_val_loss`` is the mean of ``get_kl_cc_sim_loss_wo_weight(...)["total"]``, that is NSS + CC + SIM, where larger is better:
    despite its name the rule keeps the checkpoint with the highest validation score so far, and a score that never rises above
    0.0 writes no ``best.pth`` at all.  The value is not part of a checkpoint, so a resumed run starts again from 0.0, as the
    reference does."""

    def __init__(self):
        self.min_loss = 0.0

    def is_best(self, cur_val_loss: float) -> bool:
        if cur_val_loss > self.min_loss:
            self.min_loss = cur_val_loss
            return True
        return False


def milestones(epochs: int) -> List[int]:
    """``[int(0.5 * epochs), int(0.75 * epochs)]`` (R/util/utils.py:120-121)"""
    return [int(int(epochs) * 0.5), int(0.75 * int(epochs))]


def checkpoint(model, trainer, epoch: int, step: int) -> dict:
    """The reference's checkpoint dictionary (R/diffusion_trainer.py:263-268, 408-413): ``state_dict`` is the model's,
    ``optim_dict`` is ``torch.optim.Adam``'s format (``trainer.state_dict()``), ``epoch`` the number of finished epochs.  A trainer
    built with ``ema=`` adds ``ema_dict``, its ``ema_state_dict()``; the four reference keys are what they are without it."""
    states = {"state_dict": model.state_dict(), "optim_dict": trainer.state_dict(), "epoch": int(epoch), "step": int(step)}
    if getattr(trainer, "ema", None) is not None:
        states["ema_dict"] = trainer.ema_state_dict()
    return states


def resume_from(path: str, model, trainer) -> Tuple[int, int]:
    """Loads ``state_dict`` and ``optim_dict`` of a checkpoint file (R/diffusion_trainer.py:183-190, 328-333) and returns its
    ``(epoch, step)``.  The model is loaded with ``strict=False``, as the reference does.  A trainer built with ``ema=`` also takes
    the checkpoint's ``ema_dict``; from a checkpoint without one its shadow restarts as a copy of the loaded weights with no update
    done, which is ``EMAHelper.register`` after a load."""
    states = torch.load(os.fspath(path), map_location="cpu")
    for key in ("state_dict", "optim_dict", "epoch", "step"):
        if key not in states:
            raise ValueError(f"train: {path}: a checkpoint holds state_dict, optim_dict, epoch and step; {key!r} is missing")
    model.load_state_dict(states["state_dict"], strict=False)
    trainer.load_state_dict(states["optim_dict"])
    if getattr(trainer, "ema", None) is not None:
        if "ema_dict" in states:
            trainer.load_ema_state_dict(states["ema_dict"])
        else:
            trainer.reset_ema()
    return int(states["epoch"]), int(states["step"])


def load_ema_weights(path: str, model) -> dict:
    """A checkpoint's averaged weights into ``model``, for ``predict_directory`` / ``predict_av``: loads ``state_dict`` (``strict=False``,
    as ``resume_from`` does), then overwrites every parameter named in ``ema_dict["shadow"]`` with its average and tells the
    weight-pack caches of every module.  Buffers (BatchNorm running statistics) are the checkpoint's: they are not averaged.
    Returns the ``ema_dict``.  A checkpoint without one, a name the model does not have or a shape that differs raises."""
    states = torch.load(os.fspath(path), map_location="cpu")
    for key in ("state_dict", "ema_dict"):
        if key not in states:
            raise ValueError(f"train: {path}: {key!r} is missing; load_ema_weights takes a checkpoint of a trainer built with ema=")
    shadow = states["ema_dict"]["shadow"]
    params = dict(model.named_parameters())
    for name, value in shadow.items():
        if name not in params:
            raise ValueError(f"train: {path}: ema_dict names the parameter {name!r}, which the model does not have")
        if tuple(value.shape) != tuple(params[name].shape):
            raise ValueError(f"train: {path}: shadow of {name!r} has shape {tuple(value.shape)}, the parameter {tuple(params[name].shape)}")
    model.load_state_dict(states["state_dict"], strict=False)
    with torch.no_grad():
        for name, value in shadow.items():
            params[name].copy_(value)
    for m in model.modules():
        if hasattr(m, "parameters_updated"):
            m.parameters_updated()
    return states["ema_dict"]


def _ranks(group) -> Tuple[int, int]:
    if group is None:
        return 0, 1
    import torch.distributed as td

    return td.get_rank(group), td.get_world_size(group)


def _fit(model, trainer, clips: list, out_root: str, epochs: int, batch: int, size, validate, *, seed: int, decode: str,
         steps_per_load: int, threads: int, log_freq: int, resume, stop_epoch, group, prefetch: bool, load_kw: dict,
         report: FitReport, ema_validation: bool = True) -> FitReport:
    p = next(iter(model.parameters()), None)
    if p is None or not p.is_cuda:
        raise RuntimeError("diff_sal_amd train runs on the GPU only (no CPU fallback); the model is on "
                           f"{'no device (it has no parameter)' if p is None else p.device}")
    if getattr(trainer, "model", model) is not model:
        raise ValueError("train: trainer was not built around this model")
    use_ema = bool(ema_validation) and getattr(trainer, "ema", None) is not None
    _check_decode(decode, steps_per_load)
    epochs, batch, steps_per_load = int(epochs), int(batch), int(steps_per_load)
    if epochs < 1 or batch < 1 or not clips:
        raise ValueError(f"train: epochs={epochs}, batch={batch}, {len(clips)} clips")
    device, size = p.device, video_input._hw(size)
    rank, world = _ranks(group)
    writes = rank == 0
    out_root = os.fspath(out_root)
    if writes:
        os.makedirs(out_root, exist_ok=True)
    start_epoch, step = (0, 0) if resume is None else resume_from(resume, model, trainer)
    # built after the optimizer state is loaded, at the resumed epoch: the schedule goes on where the checkpoint left it (the
    # checkpoint's learning rate is the one of its last epoch, and the scheduler's first step applies a milestone that falls on
    # start_epoch)
    from torch.optim.lr_scheduler import MultiStepLR

    if start_epoch > 0:
        trainer.optimizer.param_groups[0].setdefault("initial_lr", trainer.optimizer.param_groups[0]["lr"])
    scheduler = MultiStepLR(trainer.optimizer, milestones(epochs), 0.1, last_epoch=start_epoch - 1)
    train_log = Logger(os.path.join(out_root, "train.log"), TRAIN_HEADER) if writes else None
    val_log = Logger(os.path.join(out_root, "val.log"), VAL_HEADER) if writes else None
    best = BestKeeper()
    want_audio = isinstance(clips[0], AVClip) and getattr(model, "audio_net", None) is not None
    norm = _norm(clips, load_kw.get("norm_value"), load_kw.get("mean"), load_kw.get("std"))
    audio_kw = dict(window=load_kw.get("window"), resample=load_kw.get("resample", "kaiser_best"))
    last = epochs if stop_epoch is None else min(int(stop_epoch), epochs)
    pool = ThreadPoolExecutor(max_workers=1) if prefetch else None
    try:
        for epoch in range(start_epoch, last):
            order = epoch_order(len(clips), epoch, seed, rank, world, batch)
            loads = [order[lo:lo + steps_per_load] for lo in range(0, len(order), steps_per_load)]
            meters = DeviceMeters(device)
            lr = trainer.optimizer.param_groups[0]["lr"]

            def host(k):
                return _host_load(clips, loads[k], decode, threads, want_audio)

            pending = pool.submit(host, 0) if pool is not None and loads else None
            for k in range(len(loads)):
                load = pending.result() if pending is not None else host(k)
                # the next load's files are read (and, with decode="host", decoded) on host threads while these steps train
                pending = pool.submit(host, k + 1) if pool is not None and k + 1 < len(loads) else None
                for b in _device_load(clips, load, size, device, decode, norm, audio_kw):
                    cond = {"img": b["img"]}
                    if "audio" in b:
                        cond["audio"] = b["audio"]
                    loss = trainer.step(b["salmap"], cond, sample_ids=b["sample_ids"] if trainer.noise_source == "device" else None)
                    step += 1
                    losses = trainer.last_losses if trainer.last_losses is not None else {n: (loss if n in ("total", "main") else 0.0)
                                                                                             for n in LOSS_NAMES}
                    meters.update(losses)
                    if writes and log_freq and step % int(log_freq) == 1:      # R/diffusion_trainer.py:238-241, 379
                        m = meters.means()
                        print("Epoch: [{}/{}][{}/{}]\tTotal Step: {}\tLoss: {:.4f}\tCC {:.3f}\tSIM {:.3f}\tNSS {:.3f}\tMAIN {:.3f}".format(
                            epoch + 1, epochs, meters.count, len(order), step, m["total"], m["cc"], m["sim"], m["nss"], m["main"]))
            row = train_row(epoch + 1, step, meters.means(), lr)
            report.train_rows.append(row)
            states = checkpoint(model, trainer, epoch + 1, step)
            if writes:
                train_log.log(row)
                path = os.path.join(out_root, "ckpt_{}.pth".format(epoch + 1))
                torch.save(states, path)
                report.checkpoints.append(path)
            if validate is not None:
                # the checkpoint above holds the raw weights; val.log and the choice of best.pth refer to the average
                with trainer.ema_weights() if use_ema else contextlib.nullcontext():
                    val = validate()
                vrow = val_row(epoch + 1, step, val.losses)
                report.val_rows.append(vrow)
                if writes:
                    val_log.log(vrow)
                if best.is_best(val.losses["total"]):
                    report.best_epochs.append(epoch + 1)
                    if writes:
                        torch.save(states, os.path.join(out_root, "best.pth"))
            scheduler.step()
            report.epochs.append(epoch + 1)
    finally:
        if pool is not None:
            pool.shutdown(wait=True)
        for log in (train_log, val_log):
            if log is not None:
                log.close()
    report.step = step
    return report


def fit_directory(model, trainer, data_type: str, root: str, out_root: str, epochs: int, batch: int, *, size=video_input.SAMPLE_SIZE,
                  sampler=None, val_root: Optional[str] = None, val_batch: Optional[int] = None, loss_config=None, seed: int = 0,
                  decode: str = DEFAULT_DECODE, steps_per_load: int = DEFAULT_STEPS_PER_LOAD, threads: int = 16, log_freq: int = 0,
                  resume: Optional[str] = None, stop_epoch: Optional[int] = None, group=None, prefetch: bool = True,
                  videos: Optional[Sequence] = None, val_videos: Optional[Sequence] = None, len_snippet: int = 32, alternate: int = 1,
                  norm_value=None, mean=None, std=None, ema_validation: bool = True) -> FitReport:
    """The reference's ``train()`` (R/diffusion_trainer.py:300-432) for ``list_train_clips(data_type, root, len_snippet=...,
    alternate=..., videos=videos)``.  ``trainer`` is the caller's ``DiffusionTrainStep`` around ``model``: ``loss_config``,
    ``noise_source``, ``t_mode`` and ``training_target`` are theirs.  Per epoch, from ``resume``'s epoch on:

    * the batches of ``epoch_order(len(clips), epoch, seed, rank, world, batch)`` go through ``load_batches``' front end,
      ``steps_per_load`` steps per call with ``decode`` (defaults: ``DEFAULT_STEPS_PER_LOAD``, ``DEFAULT_DECODE``, chosen from the
      measurements in DESIGN.md), and ``trainer.step(salmap, {"img": img}, sample_ids=...)``; with ``prefetch`` the next load's
      files are read on host threads meanwhile.  The sample ids are the clips' positions in the listing;
    * the five loss values of every step (``trainer.last_losses``; the built-in MSE counts as ``main`` and ``total``) are added
      to device meters, read every ``log_freq`` steps (0: never) for a printed line and at the epoch's end for the ``train.log``
      row ``epoch, total_step, loss, main, cc, sim, nss, lr`` with ``round(..., 3)``;
    * ``ckpt_<epoch>.pth`` is ``{"state_dict", "optim_dict", "epoch", "step"}``, the reference's format;
    * with a ``sampler`` (a ``DiffusionSampler`` around ``model``), ``predict.predict_directory(model, sampler, data_type,
      val_root or root, None, losses=True, ...)`` validates without writing files; its rounded means are the ``val.log`` row and
      ``best.pth`` follows ``BestKeeper``'s rule;
    * ``MultiStepLR(trainer.optimizer, [int(0.5 * epochs), int(0.75 * epochs)], 0.1)`` is stepped once.

    ``stop_epoch`` ends the run after that many epochs of the ``epochs`` the schedule is laid out for; ``resume`` names a
    ``ckpt_<k>.pth`` and restores both dictionaries, the epoch and the step, so that stopping and resuming gives the uninterrupted
    run's parameters and moments.  ``group``: ``epoch_order`` shards the listing over its ranks and rank 0 writes; the
    validation shards its videos as ``predict_directory`` does.  Returns a ``FitReport``.

    A trainer built with ``ema=`` has its average saved and restored (``ema_dict`` of the checkpoint) and, unless
    ``ema_validation=False``, validated: ``validate`` runs inside ``trainer.ema_weights()``, so ``val.log`` and the choice of
    ``best.pth`` refer to the averaged weights (the file itself holds the raw weights and the shadow; ``load_ema_weights`` is the
    route from it to a prediction with the average).

    A trainer built with ``hip_graph=True`` works as it is: the loop calls ``trainer.step`` and reads ``trainer.last_losses`` and
    nothing else.  Its loss tensors are static, overwritten by the next step in stream order; the meters add them to their device
    sums right after each step, on the same stream, so they read every step's own values.  The front end's uploads run on the
    loop's thread between steps, never during a capture, and the prefetch thread only reads and decodes files on the host."""
    clips = list_train_clips(data_type, root, len_snippet=len_snippet, alternate=alternate, videos=videos)
    validate = None
    if sampler is not None:
        def validate():
            return predict.predict_directory(model, sampler, data_type, root if val_root is None else val_root, None,
                                             batch=batch if val_batch is None else val_batch, size=size, videos=val_videos, losses=True,
                                             loss_config=loss_config, group=group, threads=threads, write=False, len_snippet=len_snippet,
                                             alternate=alternate)
    return _fit(model, trainer, clips, out_root, epochs, batch, size, validate, seed=seed, decode=decode, steps_per_load=steps_per_load,
                threads=threads, log_freq=log_freq, resume=resume, stop_epoch=stop_epoch, group=group, prefetch=prefetch,
                load_kw=dict(norm_value=norm_value, mean=mean, std=std), report=FitReport(), ema_validation=ema_validation)


def fit_av(model, trainer, sets: Sequence, out_root: str, epochs: int, batch: int, *, size=video_input.SAMPLE_SIZE, sampler=None,
           val_sets: Optional[Sequence] = None, val_batch: Optional[int] = None, loss_config=None, seed: int = 0,
           decode: str = DEFAULT_DECODE, steps_per_load: int = DEFAULT_STEPS_PER_LOAD, threads: int = 16, log_freq: int = 0,
           resume: Optional[str] = None, stop_epoch: Optional[int] = None, group=None, prefetch: bool = True, drop_empty: bool = True,
           sample_duration: int = predict.CLIP_FRAMES, step_duration: int = 90, window: Optional[int] = None,
           resample="kaiser_best", ema_validation: bool = True) -> FitReport:
    """The loop of the reference's ``train_av_data()`` (R/diffusion_trainer.py:139-298) for one split.  ``sets`` is a list of
    ``(video_root, fold_list, salmap_root, audio_root)``; their ``list_av_train_clips`` listings are concatenated in that order, as
    ``get_training_av_loader`` concatenates its six datasets (R/datasets/prepare_data.py:131-139).  Everything else is as in
    ``fit_directory``, with these differences:

    * ``drop_empty`` (default): ``drop_empty_maps`` removes the clips whose target map is all zero from the listing before the
      first epoch, and ``FitReport.removed`` lists them.  The reference replaces such a clip by a random other item whenever it is
      drawn; this is the deliberate difference named in the module's docstring;
    * the condition holds ``audio`` when the model has an ``audio_net`` (``load_batches``);
    * with a ``sampler``, every set of ``val_sets`` (same four paths; default: none) is validated with ``predict.predict_av(...,
      losses=True)`` without files, and the ``val.log`` row holds the means over all their chunks.

    A trainer built with ``hip_graph=True`` works as it is (see ``fit_directory``)."""
    clips: list = []
    for s in sets:
        clips += list_av_train_clips(*s, sample_duration=sample_duration, step_duration=step_duration)
    report = FitReport()
    if drop_empty and clips:
        p = next(iter(model.parameters()), None)
        clips, report.removed = drop_empty_maps(clips, size, device=None if p is None else p.device, decode=decode, threads=threads)
    validate = None
    if sampler is not None and val_sets:
        def validate():
            total, chunks = {k: 0.0 for k in LOSS_NAMES}, 0
            for s in val_sets:
                r = predict.predict_av(model, sampler, tuple(s), None, batch=batch if val_batch is None else val_batch, size=size,
                                       losses=True, loss_config=loss_config, group=group, window=window, resample=resample,
                                       threads=threads, write=False)
                for k in LOSS_NAMES:
                    total[k] += r.losses[k] * r.chunks if r.chunks else 0.0
                chunks += r.chunks
            return predict.Report(losses={k: (total[k] / chunks if chunks else float("nan")) for k in LOSS_NAMES}, chunks=chunks)
    return _fit(model, trainer, clips, out_root, epochs, batch, size, validate, seed=seed, decode=decode, steps_per_load=steps_per_load,
                threads=threads, log_freq=log_freq, resume=resume, stop_epoch=stop_epoch, group=group, prefetch=prefetch,
                load_kw=dict(window=window, resample=resample), report=report, ema_validation=ema_validation)
