"""The reference's clip listings restated for the tests of ``diff_sal_amd.predict``, with the lines they restate.  torchvision is
not installed where the tests run, so the dataset classes themselves cannot be imported; this file follows them rule by rule and
returns plain tuples ``(video, [frame file names], gt_index, map file name)``, names relative to the video's folders.  Written
apart from ``predict.list_clips`` on purpose: explicit loops, no shared helper."""
import os
from decimal import ROUND_HALF_UP, Decimal, localcontext
from statistics import median


def frame_numbers(start, alternate, len_snippet, first):
    # R/datasets/dhf1k_data.py:70-74, ucf_dataset.py:57-61 (first = 1); holly2wood_dataset.py:62-66 (first = 0)
    count = 16 if len_snippet > 16 else len_snippet
    return [start + alternate * i + first for i in range(count)]


def centre_one(arr):
    # get_center_slice(arr, 1): R/datasets/dhf1k_data.py:84-88
    c = len(arr) // 2
    s = c - 1 // 2
    return arr[s:s + 1][0]


def dhf1k_val(root, len_snippet, alternate=1, gt_length=1):
    # R/datasets/dhf1k_data.py:28-30, 40-47: names sorted as integers, the validation block; here by name 601 .. 700
    frames = os.path.join(root, "frames")
    out = []
    for v in sorted(os.listdir(frames), key=int):
        if not 601 <= int(v) <= 700:
            continue
        n = len(os.listdir(os.path.join(frames, v)))
        for i in range(0, n - alternate * len_snippet, gt_length):
            nums = frame_numbers(i, alternate, len_snippet, 1)
            g = centre_one(nums)                                       # :92
            out.append((v, ["%d.png" % k for k in nums], g, "%04d.png" % g))      # :78; R/datasets/meta_data.py:73
    return out


def testing_starts(n, len_snippet, alternate, gt_length):
    # R/datasets/ucf_dataset.py:38-42, holly2wood_dataset.py:40-44: None for a video that is skipped
    if n < alternate * len_snippet:
        return None
    starts = []
    for i in range(0, n - alternate * len_snippet, gt_length):
        starts.append(i)
    starts.append(n - len_snippet)
    return starts


def ucf_test(root, len_snippet, alternate=1, gt_length=1):
    base = os.path.join(root, "testing")                               # R/datasets/ucf_dataset.py:33
    out = []
    for v in sorted(os.listdir(base)):
        starts = testing_starts(len(os.listdir(os.path.join(base, v, "images"))), len_snippet, alternate, gt_length)
        if starts is None:
            continue
        pieces = v.split("-")                                          # :64; the name is everything in front of the last hyphen
        name, number = "-".join(pieces[:-1]), pieces[-1]
        for i in starts:
            nums = frame_numbers(i, alternate, len_snippet, 1)
            g = centre_one(nums)                                       # :82
            out.append((v, ["{}_{}_{:03d}.png".format(name, number, k) for k in nums], g, "{}_{}_{:03d}.png".format(name, number, g)))      # :68, :85
    return out


def holly_test(root, len_snippet, alternate=1, gt_length=1):
    base = os.path.join(root, "testing")                               # R/datasets/holly2wood_dataset.py:35
    out = []
    for v in sorted(os.listdir(base)):
        listing = sorted(os.listdir(os.path.join(base, v, "images")))  # :69
        starts = testing_starts(len(listing), len_snippet, alternate, gt_length)
        if starts is None:
            continue
        for i in starts:
            pos = frame_numbers(i, alternate, len_snippet, 0)
            g = centre_one(pos)                                        # :85
            out.append((v, [listing[k] for k in pos], g, listing[g]))  # :71, :88
    return out


def av_exhaustive(n_frames, sample_duration=16):
    """``[(frame numbers after TemporalCenterCrop, median)]`` of one video: R/datasets/saliency_db.py:244-248 with step 1 and
    step_duration = sample_duration (:269-272), R/datasets/temporal_transforms.py:34-53, saliency_db.py:369-372"""
    out = []
    for j in range(1, n_frames, 1):
        idx = list(range(j, min(n_frames + 1, j + sample_duration)))
        c = len(idx) // 2
        b = max(0, c - sample_duration // 2)
        e = min(b + sample_duration, len(idx))
        crop = idx[b:e]
        k = 0
        while len(crop) < sample_duration:                             # the walk reads what it appends
            crop.append(crop[k])
            k += 1
        with localcontext() as ctx:
            ctx.rounding = ROUND_HALF_UP
            med = int(Decimal(median(crop)).to_integral_value())
        out.append((crop, med))
    return out
