"""From a dataset folder to the folder of prediction files ``evaluate.score_directory`` reads: the reference trainer's ``test()``
and ``test_av_data()`` loops (R/diffusion_trainer.py:714-765, 823-896) with its dataset classes' listing rules, over the stages
this package already has.  No kernel is new here; the hot path is the existing ones, composed:

    frame files --png / jpeg.decode--> uint8 frames --video_input.transform_frames--> resized frames (once per frame)
      --gather_clips--> img [B, 3, 16, h, w] --DiffusionSampler.sample_image--> pred [B, 1, h, w]
      --png / jpeg.save_predictions--> <out_root>/<video>/<gt_index>.png  |  <out_root>/<set>/<video>/pred_sal_%06d.jpg

Only file bytes travel between host and device: no pixel is touched on the host.

* ``list_clips`` / ``list_av_clips`` are the listings (host code: folders are listed, no file is opened);
* ``predict_directory`` is ``test()`` for DHF1K, UCF-Sports and Hollywood-2, ``predict_av`` is ``test_av_data()`` for the
  audio-visual sets;
* ``read_wav`` reads a ``.wav`` with the standard library.

**Clip ids.**  With ``DiffusionSampler(noise_source="device")`` the noise of a clip is keyed by its id, and the drivers pass

    clip_id(video, gt_index) = crc32(video name as UTF-8) * 2^31 + gt_index

(``video`` as it names the output folder, for the audio-visual sets ``"<set>/<video>"`` before the renaming; ``gt_index`` below
2^31; the id is below 2^63).  It is a pure function of (video, gt_index), so with the sampler's default ``clip_passes`` a
prediction does not depend on ``batch``, on the number of ranks or on the order of the videos.  Two videos whose names share a
CRC-32 would share their noise; that is harmless for a prediction and has a chance of 2^-32 per pair.

Differences from the reference's loops, all deliberate:

* the reference's ``prepare_data`` pads the last batch by repeating its last clip and its loader drops an incomplete one; the
  drivers do neither: the short last chunk of a video is evaluated as it is, and a chunk never spans two videos (so the
  loss means, which weigh every chunk alike, are those of these chunks, not of the reference's batches);
* ``inverse_data_transform``'s clamp to [0, 1] (R/diffusion_trainer.py:739) is not applied: the files hold
  ``postprocess.to_uint8(sample_image(...))``, and the losses see that prediction;
* videos are walked in sorted order where the reference takes ``os.listdir``'s;
* for the audio-visual sets a clip whose target map is all zero is skipped and reported; the reference's dataset returns a random
  other item in its place (R/datasets/saliency_db.py:390-392), so it writes no file for that frame either, and rewrites another.

GPU only: a CPU model raises.
"""
from __future__ import annotations

import os
import wave
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _image_files, video_input

Tensor = torch.Tensor

DATA_TYPES = ("dhf1k", "ucf", "holly")
CLIP_FRAMES = 16                                   # the datasets' cap: a len_snippet above 16 still reads 16 frames
DHF1K_VAL = range(601, 701)                        # video_names[600:700] of the complete set, R/datasets/dhf1k_data.py:28-30
# save_img's data_convert_dict, R/diffusion_trainer.py:912-919
AV_FOLDERS = {"AVAD": "avad", "Coutrot_db1": "coutrot1", "Coutrot_db2": "coutrot2", "DIEM": "diem", "ETMD_av": "etmd", "SumMe": "summe"}
AV_PRE_SIZE = video_input.PRE_SIZE                 # pil_loader's img.resize((320, 240))
LOSS_NAMES = ("main", "cc", "sim", "nss", "total")  # R/diffusion_trainer.py:731


@dataclass(frozen=True)
class Clip:
    """One item of a visual set's listing: the 16 frame files, the index that names the output file and the annotation map."""
    video: str
    frame_files: Tuple[str, ...]
    gt_index: int
    gt_file: str


@dataclass(frozen=True)
class AVClip:
    """One item of an audio-visual listing.  ``frame_indices`` are the 1-based frame numbers after the temporal centre crop (16 of
    them, a short tail walked again from its head); ``gt_index`` is their median; ``video_id`` is ``"<set>/<video>"``."""
    video: str
    video_id: str
    frame_indices: Tuple[int, ...]
    frame_files: Tuple[str, ...]
    gt_index: int
    gt_file: str
    wav_file: str
    n_frames: int
    fps: float


@dataclass
class Report:
    """What a driver did: ``clips`` predicted, the ``files`` written (paths, in order), ``skipped`` as (video, gt_index, reason) and,
    with ``losses=True``, the means ``{"main", "cc", "sim", "nss", "total"}`` (``chunks``: how many values each mean is of)."""
    clips: int = 0
    files: List[str] = field(default_factory=list)
    skipped: List[Tuple[str, int, str]] = field(default_factory=list)
    losses: Optional[Dict[str, float]] = None
    chunks: int = 0


# ---- listings (host) ----------------------------------------------------------------------------------------------------

def _starts(n: int, len_snippet: int, alternate: int, gt_length: int, extra: bool) -> List[int]:
    starts = list(range(0, n - alternate * len_snippet, gt_length))
    if extra:
        starts.append(n - len_snippet)
    return starts


def _centre(indices: Sequence[int]) -> int:
    """``get_center_slice(indices, 1)[0]`` (R/datasets/dhf1k_data.py:84-88): element ``len // 2``, element 8 of 16"""
    return indices[len(indices) // 2]


def list_clips(data_type: str, root: str, *, len_snippet: int = 32, gt_length: int = 1, alternate: int = 1,
               videos: Optional[Sequence] = None) -> List[Clip]:
    """The reference's ``mode="val"`` listing of a visual set under ``root``, in its order: per video, every start in turn.

    Quirks of the reference that are kept:

    * a ``len_snippet`` above 16 still reads 16 frames per clip (R/datasets/dhf1k_data.py:70-74) but enters the range of starts,
      so it shortens the listing: ``len_snippet=32`` on 40 frames gives starts 0 .. 7;
    * ``dhf1k`` (R/datasets/dhf1k_data.py:40-47, 70-74, 84-99): video folders of ``<root>/frames``; starts
      ``range(0, n - alternate * len_snippet, gt_length)`` with ``n`` the number of entries of the folder; frame files
      ``'%d.png' % (start + alternate * i + 1)`` (``video_input.dhf1k_indices``); ``gt_index`` is element 8 of those numbers; the
      map is ``<root>/maps/<video>/%04d.png`` of it (R/datasets/meta_data.py:70-77).  A video of exactly
      ``alternate * len_snippet`` frames gives no clip;
    * ``ucf`` (R/datasets/ucf_dataset.py:32-43, 57-68, 73-94) and ``holly`` (R/datasets/holly2wood_dataset.py:34-45, 62-73, 77-98):
      videos of ``<root>/testing``, frames in ``<video>/images``, maps in ``<video>/maps``; a video with fewer than
      ``alternate * len_snippet`` frames is skipped; after the range of starts one extra clip starts at ``n - len_snippet`` (with
      ``alternate`` above 1 its last frame numbers lie past the video's end: the reference fails on that file, and so does a driver
      here);
    * ``ucf`` frames and maps are ``<name>_<clip>_%03d.png`` of the 1-based numbers, ``gt_index`` element 8 of them;
    * ``holly`` indices are 0-based positions ``start + alternate * i`` in the sorted listing of ``images``; ``gt_index`` is that
      0-based position and names the output ``<gt_index>.png``, and the map is the file of the same name in ``maps``.  (The
      reference's scorer then reads ``<k>.png`` as the k-th map counted from 1, ``evaluate.pair_files``: the two disagree by one
      frame in the reference, and both are restated as they are.)

    Differences, deliberate:

    * the ``ucf`` video name is taken apart at its last hyphen (``Diving-Side-001`` -> ``Diving-Side``, ``001``).  The reference
      calls ``file_name.strip("-001")``, which removes *characters* of that set from both ends, not a suffix: it agrees for the
      names of the set and would mangle a name that begins or ends with ``-``, ``0`` or ``1`` in front of the hyphen;
    * ``dhf1k`` takes the folders whose integer name is 601 .. 700, in integer order; the reference takes positions 600 .. 699 of
      the integer-sorted listing, which is the same on the complete set of 1000 videos;
    * ``ucf`` / ``holly`` videos come in sorted order (the reference: ``os.listdir``'s);
    * ``videos``, when given, replaces the video list: those names, in that order;
    * ``gt_length`` other than 1 is a ValueError: the model emits one map per clip.

    No file is opened; folders are listed."""
    if data_type not in DATA_TYPES:
        raise ValueError(f"predict: data_type must be one of {DATA_TYPES}, got {data_type!r}")
    if gt_length != 1:
        raise ValueError(f"predict: gt_length must be 1 (the model emits one map per clip), got gt_length={gt_length!r}")
    len_snippet, alternate = int(len_snippet), int(alternate)
    if len_snippet < 1 or alternate < 1:
        raise ValueError(f"predict: len_snippet and alternate must be at least 1, got {len_snippet}, {alternate}")
    root = os.fspath(root)
    clips: List[Clip] = []
    if data_type == "dhf1k":
        img_path, ann_path = os.path.join(root, "frames"), os.path.join(root, "maps")
        if videos is None:
            videos = sorted((v for v in os.listdir(img_path) if v.isdigit() and int(v) in DHF1K_VAL), key=int)
        for v in (str(v) for v in videos):
            n = len(os.listdir(os.path.join(img_path, v)))
            for start in _starts(n, len_snippet, alternate, 1, extra=False):
                numbers = video_input.dhf1k_indices(start, alternate, len_snippet)
                gt = _centre(numbers)
                clips.append(Clip(v, tuple(os.path.join(img_path, v, "%d.png" % i) for i in numbers), gt,
                                  os.path.join(ann_path, v, "%04d.png" % gt)))
        return clips
    base = os.path.join(root, "testing")
    if videos is None:
        videos = sorted(os.listdir(base))
    for v in (str(v) for v in videos):
        images, maps = os.path.join(base, v, "images"), os.path.join(base, v, "maps")
        names = sorted(os.listdir(images))
        n = len(names)
        if n < alternate * len_snippet:
            continue
        if data_type == "ucf":
            name, sep, number = v.rpartition("-")
            if not sep:
                raise ValueError(f"predict: ucf video {v!r} has no hyphen to take its name apart at")
        for start in _starts(n, len_snippet, alternate, 1, extra=True):
            if data_type == "ucf":
                numbers = video_input.dhf1k_indices(start, alternate, len_snippet)      # the same 1-based numbers
                gt = _centre(numbers)
                files = ["{}_{}_{:03d}.png".format(name, number, i) for i in numbers]
                gt_name = "{}_{}_{:03d}.png".format(name, number, gt)
            else:
                positions = [i - 1 for i in video_input.dhf1k_indices(start, alternate, len_snippet)]
                gt = _centre(positions)
                if positions[-1] >= n:
                    raise ValueError(f"predict: holly video {v!r}: the clip at start {start} reads position {positions[-1]} of {n} frames")
                files = [names[i] for i in positions]
                gt_name = names[gt]
            clips.append(Clip(v, tuple(os.path.join(images, f) for f in files), gt, os.path.join(maps, gt_name)))
    return clips


def read_fold_list(path: str) -> List[Tuple[str, int, float]]:
    """``read_sal_text`` (R/datasets/saliency_db.py:80-88): the ``name nframes fps`` lines of a fold list"""
    out = []
    with open(path, "r") as f:
        for line in f:
            word = line.split()
            if word:
                out.append((word[0], int(word[1]), float(word[2])))
    return out


def list_av_clips(video_root: str, fold_list: str, salmap_root: str, audio_root: str, *, sample_duration: int = CLIP_FRAMES) -> List[AVClip]:
    """The exhaustive listing of ``saliency_db_spec(exhaustive_sampling=True)`` (R/datasets/saliency_db.py:173-252, 269-272,
    318-324, 369-380): for every ``name nframes fps`` line of ``fold_list``, skipping a video without its frame folder
    ``<video_root>/<name>``, without ``<salmap_root>/<name>/maps``, without ``<audio_root>/<name>/<name>.wav`` or with
    ``nframes <= 1``, one clip per ``j in range(1, nframes)`` with the frame numbers ``range(j, min(nframes + 1, j + 16))``, then
    ``video_input.center_crop_indices`` (which pads a short tail by walking it again) and ``video_input.median_index`` for the
    frame that labels the clip.  Files: ``img_%05d.jpg``, ``maps/eyeMap_%05d.jpg``.  The set's name is the last component of
    ``video_root`` (the reference's ``path.split('/')[-2]``).  The ``.wav`` is not opened here."""
    video_root = os.fspath(video_root).rstrip("/" + os.sep)
    dataset = os.path.basename(video_root)
    sample_duration = int(sample_duration)
    clips: List[AVClip] = []
    for name, n_frames, fps in read_fold_list(fold_list):
        video_path = os.path.join(video_root, name)
        annot_path = os.path.join(salmap_root, name, "maps")
        wav_path = os.path.join(audio_root, name, name + ".wav")
        if not os.path.exists(video_path) or not os.path.exists(annot_path) or n_frames <= 1 or not os.path.exists(wav_path):
            continue
        for j in range(1, n_frames):
            idx = video_input.center_crop_indices(range(j, min(n_frames + 1, j + sample_duration)), sample_duration)
            med = video_input.median_index(idx)
            clips.append(AVClip(name, f"{dataset}/{name}", tuple(idx), tuple(os.path.join(video_path, "img_{:05d}.jpg".format(i)) for i in idx),
                                med, os.path.join(annot_path, "eyeMap_{:05d}.jpg".format(med)), wav_path, n_frames, fps))
    return clips


def read_wav(path: str) -> Tuple[np.ndarray, int]:
    """``(samples int16 [n], rate)`` of a ``.wav`` file, read on the host with the standard library.  The file must be 16-bit PCM
    and mono (what the reference's ``sf.read(..., dtype='int16')`` feeds a one-dimensional excerpt with); anything else is a
    ValueError naming the file."""
    try:
        with wave.open(os.fspath(path), "rb") as w:
            channels, width, rate, n = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
            if w.getcomptype() != "NONE":
                raise ValueError(f"predict: {path}: compression {w.getcomptype()!r}; 16-bit PCM only")
            if width != 2:
                raise ValueError(f"predict: {path}: {8 * width}-bit samples; 16-bit PCM only")
            if channels != 1:
                raise ValueError(f"predict: {path}: {channels} channels; mono only")
            data = w.readframes(n)
    except wave.Error as e:
        raise ValueError(f"predict: {path}: not a PCM .wav file ({e})") from None
    return np.frombuffer(data, dtype="<i2").astype(np.int16), int(rate)


def clip_id(video, gt_index: int) -> int:
    """The id that keys a clip's device noise: ``crc32(video name) * 2^31 + gt_index`` (see the module's docstring)."""
    g = int(gt_index)
    if not 0 <= g < 1 << 31:
        raise ValueError(f"predict: gt_index {g} outside 0 .. 2^31 - 1")
    return zlib.crc32(str(video).encode("utf-8")) * (1 << 31) + g


# ---- drivers ------------------------------------------------------------------------------------------------------------

def _checked(model, sampler, batch, size) -> Tuple[torch.device, int, Tuple[int, int]]:
    p = next(iter(model.parameters()), None)
    if p is None or not p.is_cuda:
        raise RuntimeError("diff_sal_amd predict runs on the GPU only (no CPU fallback); the model is on "
                           f"{'no device (it has no parameter)' if p is None else p.device}")
    if getattr(model, "module", model) is not sampler.model:
        raise ValueError("predict: sampler was not built around this model")
    if int(batch) < 1:
        raise ValueError(f"predict: batch must be at least 1, got {batch}")
    return p.device, int(batch), video_input._hw(size)


def _positions(clips: Sequence) -> Tuple[List[str], List[List[int]]]:
    """the files any clip reads, each once in order of first use, and every clip as positions in that list"""
    where: Dict[str, int] = {}
    rows = []
    for c in clips:
        rows.append([where.setdefault(f, len(where)) for f in c.frame_files])
    return list(where), rows


def _by_video(clips: Sequence) -> List[Tuple[str, list]]:
    """the clips grouped per video, videos in order of first appearance, a video's clips in list order"""
    groups: Dict[str, list] = {}
    for c in clips:
        groups.setdefault(c.video, []).append(c)
    return list(groups.items())


def _shard(items: list, group) -> list:
    import torch.distributed as td

    from . import dist

    if group is None:
        return items
    own = dist.shard_range(len(items), td.get_rank(group), td.get_world_size(group))
    return items[own.start:own.stop]


class _Meter:
    """``AverageMeterList`` (R/util/utils.py:37-53): every update rounds the value to 3 places and weighs it alike"""

    def __init__(self):
        self.sums = {k: 0.0 for k in LOSS_NAMES}
        self.count = 0

    def update(self, d) -> None:
        for k in LOSS_NAMES:
            self.sums[k] += round(d[k].item(), 3)
        self.count += 1

    def means(self, device, group) -> Tuple[Dict[str, float], int]:
        t = torch.tensor([self.sums[k] for k in LOSS_NAMES] + [float(self.count)], dtype=torch.float64)
        if group is not None:
            import torch.distributed as td

            t = t.to(device)
            td.all_reduce(t, group=group)
            t = t.cpu()
        n = int(t[-1])
        return {k: (float(t[i]) / n if n else float("nan")) for i, k in enumerate(LOSS_NAMES)}, n


def _sample(sampler, img, audio, ids, device):
    if sampler.noise_source == "device":
        return sampler.sample_image(None, img=img, audio=audio, clip_ids=ids)
    x = torch.randn(sampler._state_shape(img.shape[0]), device=device)      # R/diffusion_trainer.py:119
    return sampler.sample_image(x, img=img, audio=audio)


class _eval_mode:
    """``self.model.eval()`` of the reference's loops, undone afterwards"""

    def __init__(self, model):
        self.model, self.was = model, model.training

    def __enter__(self):
        self.model.eval()

    def __exit__(self, *exc):
        self.model.train(self.was)


@torch.no_grad()
def predict_directory(model, sampler, data_type: str, root: str, out_root: str, *, batch: int = 4, size=video_input.SAMPLE_SIZE,
                      fmt: str = "png", videos: Optional[Sequence] = None, losses: bool = False, loss_config=None, group=None,
                      norm_value=255, mean=video_input.IMAGENET_MEAN, std=video_input.IMAGENET_STD, threads: int = 16,
                      write: bool = True, **list_kwargs) -> Report:
    """The reference's ``test()`` (R/diffusion_trainer.py:714-765) for ``list_clips(data_type, root, videos=videos,
    **list_kwargs)``: writes ``<out_root>/<video>/<gt_index>.png`` for every clip, the layout ``evaluate.pair_files`` expects under
    a task folder, and returns a ``Report``.

    Per video: the bytes of every frame file any of its clips uses are read once (``threads`` host threads, at most 16), decoded in
    one ``png.decode(..., "RGB")`` call and resized once per frame (``video_input.transform_frames(frames, size)``; a video's
    decoded frames are in device memory together: 0.7 MB per 360 x 640 frame).  Its clips are then walked in list order in chunks of
    ``batch``: ``video_input.gather_clips`` (``ToTensor`` + ``Normalize`` with ``norm_value`` / ``mean`` / ``std``, by default
    R/datasets/meta_data.py:27-31's), ``sampler.sample_image(x, img=clip, clip_ids=...)`` with ``x = None`` and
    ``clip_id(video, gt_index)`` for a sampler with ``noise_source="device"`` and ``x = torch.randn`` for ``"torch"``
    (R/diffusion_trainer.py:119), then ``png.save_predictions`` (``fmt="png"``, encoded on the device) or
    ``postprocess.save_predictions`` (``fmt="pillow"``, the same pixels through Pillow on the host).  The short last chunk of a
    video is evaluated as it is: nothing is padded, nothing dropped (the reference does both, see the module's docstring).

    ``losses=True`` also decodes the clips' map files (``"L"``), builds the targets with ``video_input.target_maps(maps, size)`` and
    accumulates ``sal_losses.get_kl_cc_sim_loss_wo_weight(loss_config, pred, target)`` as the reference's ``AverageMeterList`` does
    (R/util/utils.py:47-50: every chunk's value rounded to 3 places, every chunk weighed alike); ``Report.losses["total"]`` is what
    ``test()`` returns and a training loop picks ``best.pth`` by.  ``loss_config=None`` leaves ``main`` (the KL term) at zero.

    ``group`` (a ``torch.distributed`` process group): the videos are divided over its ranks with ``dist.shard_range``, every rank
    writes its own files and reports its own clips, and the loss sums are all-reduced, so ``losses`` is the same on every rank.

    ``write=False`` writes nothing (``out_root`` is not used, ``Report.files`` stays empty): the validation pass of a training loop,
    ``save_img=False`` of the reference's ``test()``."""
    from . import png, postprocess, sal_losses

    device, batch, size = _checked(model, sampler, batch, size)
    if fmt not in ("png", "pillow"):
        raise ValueError(f"predict: fmt must be 'png' (encoded on the device) or 'pillow' (on the host), got {fmt!r}")
    save = png.save_predictions if fmt == "png" else postprocess.save_predictions
    report, meter = Report(), _Meter()
    with _eval_mode(sampler.model):
        for video, clips in _shard(_by_video(list_clips(data_type, root, videos=videos, **list_kwargs)), group):
            files, rows = _positions(clips)
            frames = png.decode(_image_files.read_files(files, threads), "RGB", device)
            resized = video_input.transform_frames(frames, size)
            del frames
            targets = None
            if losses:
                maps = png.decode(_image_files.read_files([c.gt_file for c in clips], threads), "L", device)
                targets = video_input.target_maps(maps, size)
            for lo in range(0, len(clips), batch):
                chunk = clips[lo:lo + batch]
                img = video_input.gather_clips(resized, rows[lo:lo + batch], norm_value=norm_value, mean=mean, std=std)
                pred = _sample(sampler, img, None, [clip_id(video, c.gt_index) for c in chunk], device)
                if losses:
                    meter.update(sal_losses.get_kl_cc_sim_loss_wo_weight(loss_config, pred, targets[lo:lo + batch]))
                if write:
                    report.files += save(pred, [video] * len(chunk), [c.gt_index for c in chunk], out_root)
                report.clips += len(chunk)
    if losses:
        report.losses, report.chunks = meter.means(device, group)
    return report


@torch.no_grad()
def predict_av(model, sampler, clips_or_args, out_root: str, *, batch: int = 4, size=video_input.SAMPLE_SIZE, quality: int = 95,
               losses: bool = False, loss_config=None, group=None, window: Optional[int] = None, resample="kaiser_best",
               threads: int = 16, write: bool = True) -> Report:
    """The reference's ``test_av_data()`` loop for one set and one fold (R/diffusion_trainer.py:823-896): ``clips_or_args`` is a
    list of ``AVClip`` or the ``(video_root, fold_list, salmap_root, audio_root)`` ``list_av_clips`` takes.  Writes
    ``<out_root>/<set's folder>/<video>/pred_sal_%06d.jpg`` of the clip's median frame number through ``jpeg.save_predictions`` at
    ``quality``, the set's folder renamed by the reference's table (``AV_FOLDERS``: ``AVAD`` -> ``avad``, ...; another set's name
    is a ValueError), and returns a ``Report``.

    Per video, as ``predict_directory``: the frame files any clip uses are read once, decoded in one ``jpeg.decode(..., "RGB")`` call
    and resized once per frame, ``pre_size=(240, 320)`` bicubic then ``size`` bilinear (R/datasets/saliency_db.py:29-36, 292-296);
    ``gather_clips`` applies the normalisation of R/cfgs/dataset.json:73-77.  The ``.wav`` is read on the host (``read_wav``: 16-bit
    PCM, mono, else refused by name before anything is launched) and uploaded as int16; ``audio_input.excerpt_table`` gives the
    per-frame samples at the file's rate and ``audio_input.clip_audio(..., size=(h // 2, w // 2))`` the ``audio`` input from the first
    to the last frame number of the clip; a rate other than 16 kHz goes through ``sample_rate=..., resample=resample``
    (``"kaiser_best"``: the reference's per-clip resampy step).  ``window`` defaults to the reference's ``max_audio_win``,
    ``int(22050 / 10 * 16)`` samples.  A model without an ``audio_net`` gets no audio input.

    The clips' ``eyeMap`` files are decoded (``"L"``) and made targets with ``video_input.target_maps`` whether or not losses are
    asked for: a clip whose target is all zero is skipped -- no sample, no file, no loss -- and listed in ``Report.skipped`` (one
    read-back of a flag per clip and video).  Chunks, ``clip_id("<set>/<video>", gt_index)``, ``losses``, ``loss_config``,
    ``group`` and ``write`` are as in ``predict_directory``."""
    from . import audio_input, jpeg, sal_losses

    device, batch, size = _checked(model, sampler, batch, size)
    if isinstance(clips_or_args, (tuple, list)) and len(clips_or_args) == 4 and all(isinstance(a, (str, os.PathLike)) for a in clips_or_args):
        clips_or_args = list_av_clips(*clips_or_args)
    all_clips = list(clips_or_args)
    if not all(isinstance(c, AVClip) for c in all_clips):
        raise ValueError("predict: predict_av takes a list of AVClip or (video_root, fold_list, salmap_root, audio_root)")
    folders = {}
    for c in all_clips:
        dataset = c.video_id.split("/")[0]
        if dataset not in AV_FOLDERS:
            raise ValueError(f"predict: {c.video_id!r}: set {dataset!r} is not one of {sorted(AV_FOLDERS)}")
        folders[c.video_id] = AV_FOLDERS[dataset] + "/" + c.video_id.split("/")[-1]
    videos = _shard(_by_video(all_clips), group)
    waves = {v: read_wav(clips[0].wav_file) for v, clips in videos}      # every file is checked before the first launch
    window = audio_input.DEFAULT_WINDOW if window is None else int(window)
    report, meter = Report(), _Meter()
    with _eval_mode(sampler.model):
        for video, clips in videos:
            files, rows = _positions(clips)
            frames = jpeg.decode(_image_files.read_files(files, threads), "RGB", device)
            resized = video_input.transform_frames(frames, size, pre_size=AV_PRE_SIZE, pre_filter="bicubic")
            del frames
            maps = jpeg.decode(_image_files.read_files([c.gt_file for c in clips], threads), "L", device)
            targets = video_input.target_maps(maps, size)
            blank = (targets.flatten(1).amax(1) == 0).cpu().tolist()
            kept = []
            for i, c in enumerate(clips):
                if blank[i]:
                    report.skipped.append((c.video_id, c.gt_index, "its target map is all zero"))
                else:
                    kept.append(i)
            samples, rate = waves[video]
            wav = torch.from_numpy(samples).to(device)
            starts, ends = audio_input.excerpt_table(clips[0].n_frames, clips[0].fps, rate, samples.shape[0])
            rate_kw = {} if rate == audio_input.SAMPLE_RATE else dict(sample_rate=rate, resample=resample)
            for lo in range(0, len(kept), batch):
                at = kept[lo:lo + batch]
                chunk = [clips[i] for i in at]
                img = video_input.gather_clips(resized, [rows[i] for i in at])
                audio = None
                if getattr(sampler.model, "audio_net", None) is not None:
                    audio = audio_input.clip_audio(wav, [int(starts[c.frame_indices[0]]) for c in chunk],
                                                   [int(ends[c.frame_indices[-1]]) for c in chunk],
                                                   size=(size[0] // 2, size[1] // 2), window=window, **rate_kw)
                pred = _sample(sampler, img, audio, [clip_id(c.video_id, c.gt_index) for c in chunk], device)
                if losses:
                    meter.update(sal_losses.get_kl_cc_sim_loss_wo_weight(loss_config, pred, targets[at]))
                if write:
                    report.files += jpeg.save_predictions(pred, [folders[c.video_id]] * len(chunk), [c.gt_index for c in chunk], out_root,
                                                          quality)
                report.clips += len(chunk)
    if losses:
        report.losses, report.chunks = meter.means(device, group)
    return report
