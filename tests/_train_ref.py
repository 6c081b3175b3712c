"""The reference's ``mode="train"`` listings, its sampler and its best-checkpoint rule restated for the tests of
``diff_sal_amd.train``, with the lines they restate.  torchvision is not installed where the tests run, so the dataset classes
themselves cannot be imported; this file follows them rule by rule and returns plain tuples ``(video, [frame file names],
gt_index, map file name)``, names relative to the video's folders.  Written apart from ``train.py`` (and from
``tests/_predict_ref.py``) on purpose: explicit loops, no shared helper."""
import os
from decimal import ROUND_HALF_UP, Decimal, localcontext
from statistics import median


def train_skip_window(len_snippet):
    # R/datasets/meta_data.py:37-41: the halving of line 38 is overwritten by line 39
    if len_snippet > 16:
        window = len_snippet // 2
        window = 16
    else:
        window = len_snippet
    return window


def train_numbers(start, alternate, len_snippet, first):
    # R/datasets/dhf1k_data.py:70-74, ucf_dataset.py:57-61 (first = 1); holly2wood_dataset.py:62-66 (first = 0)
    if len_snippet > 16:
        frame_lens = 16
        return [start + alternate * i + first for i in range(frame_lens)]
    return [start + alternate * i + first for i in range(len_snippet)]


def middle(arr):
    # get_center_slice(arr, gt_length = 1): R/datasets/dhf1k_data.py:84-88
    center = len(arr) // 2
    begin = center - 1 // 2
    end = begin + 1
    return arr[begin:end][0]


def dhf1k_train(root, len_snippet, alternate=1):
    # R/datasets/dhf1k_data.py:28-29: names sorted as integers, the first 600; here by name 1 .. 600
    frames = os.path.join(root, "frames")
    out = []
    for v in sorted(os.listdir(frames), key=int):
        if not 1 <= int(v) <= 600:
            continue
        n = len(os.listdir(os.path.join(frames, v)))                                 # :37
        for i in range(0, n - alternate * len_snippet, train_skip_window(len_snippet)):      # :38
            nums = train_numbers(i, alternate, len_snippet, 1)
            g = middle(nums)                                                         # :92
            out.append((v, ["%d.png" % k for k in nums], g, "%04d.png" % g))        # :78; R/datasets/meta_data.py:73
    return out


def ucf_train(root, len_snippet, alternate=1):
    base = os.path.join(root, "training")                                            # R/datasets/ucf_dataset.py:26
    out = []
    for v in sorted(os.listdir(base)):
        n = len(os.listdir(os.path.join(base, v, "images")))                         # :29; no skip of a short video in train mode
        pieces = v.split("-")                                                        # :64; the name is everything in front of the last hyphen
        name, number = "-".join(pieces[:-1]), pieces[-1]
        for i in range(0, n - alternate * len_snippet, train_skip_window(len_snippet)):      # :30; no extra last clip
            nums = train_numbers(i, alternate, len_snippet, 1)
            g = middle(nums)                                                         # :82
            out.append((v, ["{}_{}_{:03d}.png".format(name, number, k) for k in nums], g, "{}_{}_{:03d}.png".format(name, number, g)))      # :68, :85
    return out


def holly_train(root, len_snippet, alternate=1):
    base = os.path.join(root, "training")                                            # R/datasets/holly2wood_dataset.py:25
    out = []
    for v in sorted(os.listdir(base)):
        img_list = sorted(os.listdir(os.path.join(base, v, "images")))               # :68
        n = len(img_list)                                                            # :29
        for i in range(0, n - alternate * len_snippet, train_skip_window(len_snippet)):      # :30
            pos = train_numbers(i, alternate, len_snippet, 0)
            g = middle(pos)                                                          # :85
            out.append((v, [img_list[k] for k in pos], g, img_list[g]))             # :70, :88
    return out


def av_train(n_frames, sample_duration=16, step_duration=90):
    """``[(frame numbers after the temporal crop, median)]`` of one video of the non-exhaustive listing"""
    step = max(1, step_duration - sample_duration)                                   # R/datasets/saliency_db.py:275
    out = []
    j = 1
    while j < n_frames:                                                              # :247 range(1, n_frames, step)
        window = []
        k = j
        while k < min(n_frames + 1, j + step_duration):                              # :249-250
            window.append(k)
            k += 1
        # TemporalCenterCrop(sample_duration), R/datasets/temporal_transforms.py:34-53
        center_index = len(window) // 2
        begin_index = max(0, center_index - (sample_duration // 2))
        end_index = min(begin_index + sample_duration, len(window))
        crop = window[begin_index:end_index]
        for index in crop:
            if len(crop) >= sample_duration:
                break
            crop.append(index)
        with localcontext() as ctx:                                                  # R/datasets/saliency_db.py:369-372
            ctx.rounding = ROUND_HALF_UP
            med = int(Decimal(median(crop)).to_integral_value())
        out.append((crop, med))
        j += step
    return out


def best_epochs(values):
    """the 1-based epochs at which the reference writes ``best.pth`` for the validation values ``values``, one per epoch"""
    min_loss = 0.0                                                                   # R/diffusion_trainer.py:196, 339
    out = []
    for epoch, cur_val_loss in enumerate(values):
        if cur_val_loss > min_loss:                                                  # :276, :426
            min_loss = cur_val_loss
            out.append(epoch + 1)
    return out
