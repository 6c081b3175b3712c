"""The training front end on the GPU: the grouped resample (csrc/video_input.hip, ``video_input.resize_groups``) against the
one-size call per group and against the NumPy restatement of Pillow's resize (tests/_video_input_ref.py), and
``train.load_batches`` on trees of four videos with four geometries against the per-clip calls on Pillow-decoded frames.

Every comparison is equality: the resample is integer arithmetic, the normalisation a look-up.  Output (12, 20); the eight groups
are the smallest sources at which each path of the grouped call can go wrong (see GROUPS); the references are computed once."""
import os
import wave

import numpy as np
import pytest
import torch
from PIL import Image

from diff_sal_amd import ops, train
from diff_sal_amd import video_input as vi
from tests import _video_input_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
OUT = (12, 20)
# (H, W) of the source: what the group exercises
GROUPS = [(7, 5),        # upscale on both axes
          (33, 64),      # downscale on both axes
          (48, 21),      # mixed: rows shrink, columns (almost) keep
          (12, 20),      # a copy
          (12, 64),      # horizontal pass only
          (40, 20),      # vertical pass only
          (5, 5),        # a bicubic edge whose taps reach the border
          (97, 131)]     # the strongest downscale: the tallest span of source rows per band
PERMUTE = 7              # dst[i] = (PERMUTE * i + 3) mod total: a fixed permutation whenever total is no multiple of 7
_MEMO = {}


def _inputs(n, c):
    """the eight groups with ``n`` frames each and ``c`` channels: (host arrays, device tensors)"""
    key = ("in", n, c)
    if key not in _MEMO:
        host = [ref.noise((n, h, w, c), 100 + 10 * i + c) if i % 2 else ref.blocks((n, h, w, c), 100 + 10 * i + c, cell=3)
                for i, (h, w) in enumerate(GROUPS)]
        _MEMO[key] = host, [torch.from_numpy(a).to(DEV) for a in host]
    return _MEMO[key]


def _numpy(n, c, filt):
    """the NumPy restatement's resize of every group, concatenated in group order"""
    key = ("np", n, c, filt)
    if key not in _MEMO:
        _MEMO[key] = np.concatenate([ref.resize(a, OUT, filt) for a in _inputs(n, c)[0]])
    return _MEMO[key]


def _dst(total):
    d = [(PERMUTE * i + 3) % total for i in range(total)]
    assert sorted(d) == list(range(total)) and d != list(range(total))
    return d


@pytest.mark.parametrize("fused", [None, True, False])
@pytest.mark.parametrize("filt", ["bilinear", "bicubic"])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("n", [1, 3])
def test_grouped_resize_equals_the_calls_per_group(n, c, filt, fused):
    _, dev = _inputs(n, c)
    keep = [x.clone() for x in dev]
    per_group = torch.cat([vi.resize_u8(x, OUT, filt, fused) for x in dev])
    got = vi.resize_groups(dev, OUT, filt, fused)
    assert got.dtype == torch.uint8 and got.is_contiguous() and tuple(got.shape) == (8 * n,) + OUT + (c,)
    assert torch.equal(got, per_group)                                               # the one-size call per group
    assert np.array_equal(got.cpu().numpy(), _numpy(n, c, filt))                     # Pillow's arithmetic, restated
    assert torch.equal(vi.resize_groups(dev, OUT, filt, fused), got)                 # a second call gives the same bytes
    assert all(torch.equal(a, b) for a, b in zip(dev, keep))                         # the inputs are not modified
    # dst: a fixed permutation, given on the host and as a device tensor
    dst = _dst(8 * n)
    want = torch.empty_like(per_group)
    want[torch.tensor(dst, device=DEV)] = per_group
    assert torch.equal(vi.resize_groups(dev, OUT, filt, fused, dst=dst), want)
    assert torch.equal(vi.resize_groups(dev, OUT, filt, fused, dst=torch.tensor(dst, device=DEV)), want)
    assert torch.equal(vi.resize_groups(dev, OUT, filt, fused, dst=list(range(8 * n))), per_group)      # the identity


@pytest.mark.parametrize("c", [1, 3])
def test_one_group_equals_the_existing_call(c):
    _, dev = _inputs(3, c)
    for x in dev:
        for filt in ("bilinear", "bicubic"):
            for fused in (None, True, False):
                assert torch.equal(vi.resize_groups([x], OUT, filt, fused), vi.resize_u8(x, OUT, filt, fused))
    # the chain and the maps route a single group through the one-size calls
    assert torch.equal(vi.transform_groups([dev[1]], OUT, pre_size=(24, 32)), vi.transform_frames(dev[1], OUT, pre_size=(24, 32)))
    if c == 1:
        assert torch.equal(vi.target_maps_groups([dev[1]], OUT), vi.target_maps(dev[1], OUT))
        assert torch.equal(vi.target_maps_groups([dev[1][..., 0], dev[7]], OUT, dst=[0, 1, 2, 5, 4, 3]),
                           torch.cat([vi.target_maps(dev[1], OUT), vi.target_maps(dev[7], OUT).flip(0)]))


def test_chain_with_a_first_size_is_grouped_then_one_size():
    _, dev = _inputs(3, 3)
    want = torch.cat([vi.transform_frames(x, OUT, pre_size=(24, 32)) for x in dev])
    assert torch.equal(vi.transform_groups(dev, OUT, pre_size=(24, 32)), want)
    assert torch.equal(vi.transform_groups(dev, OUT), torch.cat([vi.transform_frames(x, OUT) for x in dev]))


def test_more_groups_than_one_launch_takes():
    """18 groups of one frame, more than ops.RESAMPLE_MAX_GROUPS: the call is split and the frames still land by dst"""
    sizes = [(5 + 3 * i, 7 + 5 * (i % 7)) for i in range(ops.RESAMPLE_MAX_GROUPS + 2)] + [OUT]
    host = [ref.noise((1, h, w, 3), 300 + i) for i, (h, w) in enumerate(sizes)]
    dev = [torch.from_numpy(a).to(DEV) for a in host]
    want = np.concatenate([ref.resize(a, OUT, "bicubic") for a in host])
    got = vi.resize_groups(dev, OUT, "bicubic")
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, torch.cat([vi.resize_u8(x, OUT, "bicubic") for x in dev]))
    dst = _dst(len(sizes))
    assert np.array_equal(vi.resize_groups(dev, OUT, "bicubic", dst=dst).cpu().numpy()[dst], want)


def test_part_filled_last_band():
    """a source so tall that the fused plan takes fewer rows per band than the output has, and a number that does not divide it"""
    for c, filt in ((3, "bilinear"), (1, "bicubic")):
        band = vi.band_rows((3960, 8), OUT, c, filt)
        assert 0 < band < OUT[0] and OUT[0] % band, (c, filt, band)
        host = [ref.noise((2, 3960, 8, c), 400 + c), ref.noise((1, 33, 64, c), 401 + c)]
        dev = [torch.from_numpy(a).to(DEV) for a in host]
        got = vi.resize_groups(dev, OUT, filt, True, dst=[2, 0, 1])
        want = np.concatenate([ref.resize(a, OUT, filt) for a in host])
        assert np.array_equal(got.cpu().numpy()[[2, 0, 1]], want)
        assert torch.equal(got[[2, 0, 1]], torch.cat([vi.resize_u8(x, OUT, filt, True) for x in dev]))


def test_launches_do_not_grow_with_the_groups():
    _, dev = _inputs(1, 3)

    def launches(groups, fused=None):
        xt = [vi.device_table(DEV, x.shape[2], OUT[1], "bilinear") for x in groups]
        yt = [vi.device_table(DEV, x.shape[1], OUT[0], "bilinear") for x in groups]
        return ops.resample_u8_groups_launches(groups, OUT[0], OUT[1], ops.FILTER_BILINEAR, xt, yt, form=vi._FORMS[fused])

    assert launches(dev) == 3                                  # fused bands, horizontal pass, vertical pass
    assert launches(dev, False) == 2 and launches(dev[3:4]) == 1 and launches(dev[:1], True) == 1
    assert launches(dev * 2) == 3                              # sixteen groups: still one launch of each form
    assert launches(dev * 2 + dev[3:4]) == 4                   # the seventeenth starts a second run


def test_arguments_are_checked_before_any_launch():
    _, dev = _inputs(1, 3)
    for bad in ([0, 1, 2, 3, 4, 5, 6, 8], [-1, 1, 2, 3, 4, 5, 6, 7]):
        with pytest.raises(ValueError, match="outside 0 .. 7"):
            vi.resize_groups(dev, OUT, dst=bad)
    with pytest.raises(ValueError, match="dst must be 8 integers"):
        vi.resize_groups(dev, OUT, dst=[0, 1, 2])
    with pytest.raises(ValueError, match="one channel count"):
        vi.resize_groups([dev[0], _inputs(1, 1)[1][1]], OUT)
    with pytest.raises(ValueError, match="non-empty sequence"):
        vi.resize_groups([], OUT)
    with pytest.raises(RuntimeError, match="GPU only"):
        vi.resize_groups([dev[0].cpu()], OUT)
    # a dst entry the host cannot see is clamped by the kernels: wrong pixels, no fault
    want = vi.resize_groups(dev, OUT)
    assert torch.equal(vi.resize_groups(dev, OUT, dst=torch.tensor([0, 1, 2, 3, 4, 5, 6, 2 ** 30], device=DEV)), want)      # clamped to 7
    assert torch.equal(vi.resize_groups(dev, OUT, dst=torch.tensor([0, 1, 2, 3, 4, 5, 6, -9], device=DEV))[1:7], want[1:7])  # to 0


# ---------------------------------------------------------------------------------------------------------- batch assembly
SIZE = (64, 128)
GEOMETRIES = [(48, 80), (40, 72), (56, 64), (48, 96)]


def picture(seed, h, w):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin((x + 3 * seed) / 9.0 + c) * np.cos((y - 2 * seed) / 7.0 + 2 * c) for c in range(3)], -1)
    return np.clip(base + rng.integers(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)


def blob(seed, h, w):
    y, x = np.mgrid[0:h, 0:w]
    cy, cx = h * (0.3 + 0.05 * (seed % 7)), w * (0.2 + 0.07 * (seed % 9))
    return np.clip(255 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * 6.0 ** 2)), 0, 255).astype(np.uint8)


def save(arr, path, **kw):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path, **kw)


def pil(files, mode):
    return torch.from_numpy(np.stack([np.asarray(Image.open(f).convert(mode)) for f in files])).to(DEV)


def write_ucf_tree(root):
    """four training videos of 34 frames with four geometries, PNG: two clips each at len_snippet 16 (starts 0 and 16); one testing
    video of 18 frames (three clips of the validation listing)"""
    for v, (h, w) in enumerate(GEOMETRIES):
        name = f"Act-{v + 1:03d}"
        for i in range(1, 35):
            save(picture(100 * v + i, h, w), os.path.join(root, "training", name, "images", f"Act_{v + 1:03d}_{i:03d}.png"))
        for g in (9, 25):
            save(blob(v + g, h, w), os.path.join(root, "training", name, "maps", f"Act_{v + 1:03d}_{g:03d}.png"))
    for i in range(1, 19):
        save(picture(900 + i, 48, 80), os.path.join(root, "testing", "Val-001", "images", f"Val_001_{i:03d}.png"))
        save(blob(i, 48, 80), os.path.join(root, "testing", "Val-001", "maps", f"Val_001_{i:03d}.png"))
    return root


def write_av_tree(root, n_frames=24, zero=("V2", 15)):
    """four videos of ``n_frames`` frames with four geometries, JPEG, with a 16 kHz wav each; the map ``zero`` is all zero.  Returns
    the four paths of a listing."""
    lines = []
    for v, (h, w) in enumerate(GEOMETRIES):
        name = f"V{v + 1}"
        for i in range(1, n_frames + 1):
            save(picture(1000 + 100 * v + i, h, w), os.path.join(root, "video", "AVAD", name, f"img_{i:05d}.jpg"), quality=90)
            m = blob(v + i, h, w)
            if (name, i) == zero:
                m = np.zeros_like(m)
            save(m, os.path.join(root, "annot", "AVAD", name, "maps", f"eyeMap_{i:05d}.jpg"), quality=90)
        rng = np.random.default_rng(50 + v)
        samples = (3000 * np.sin(np.arange(16000) * (0.05 + 0.01 * v)) + rng.integers(-500, 500, size=16000)).astype("<i2")
        os.makedirs(os.path.join(root, "audio", "AVAD", name), exist_ok=True)
        with wave.open(os.path.join(root, "audio", "AVAD", name, name + ".wav"), "wb") as f:
            f.setnchannels(1)
            f.setsampwidth(2)
            f.setframerate(16000)
            f.writeframes(samples.tobytes())
        lines.append(f"{name} {n_frames} 25.0")
    fold = os.path.join(root, "fold.txt")
    with open(fold, "w") as f:
        f.write("\n".join(lines) + "\n")
    return (os.path.join(root, "video", "AVAD"), fold, os.path.join(root, "annot", "AVAD"), os.path.join(root, "audio", "AVAD"))


@pytest.fixture(scope="module")
def ucf_tree(tmp_path_factory):
    return write_ucf_tree(str(tmp_path_factory.mktemp("ucf")))


@pytest.fixture(scope="module")
def av_tree(tmp_path_factory):
    """24 frames, step_duration 20: windows from 1, 5, 9, 13, 17, 21, labelled by frames 11, 15, 17, 17, 21, 23; the map of the second
    clip of V2 is all zero"""
    return write_av_tree(str(tmp_path_factory.mktemp("av")))


def per_clip(clips, av):
    """``clip_rgb`` / ``target_maps`` per clip on Pillow-decoded frames, with the set's loader's parameters"""
    imgs, maps = [], []
    for c in clips:
        frames = pil(c.frame_files, "RGB")
        idx = [list(range(16))]
        if av:
            imgs.append(vi.clip_rgb(frames, idx, SIZE, pre_size=(240, 320)))
        else:
            imgs.append(vi.clip_rgb(frames, idx, SIZE, norm_value=255, mean=vi.IMAGENET_MEAN, std=vi.IMAGENET_STD))
        maps.append(vi.target_maps(pil([c.gt_file], "L"), SIZE))
    return torch.cat(imgs), torch.cat(maps)


ORDER = [[0, 7], [2, 5], [6, 1]]       # three steps of two clips from different videos


def test_load_batches_on_png_files(ucf_tree):
    clips = train.list_train_clips("ucf", ucf_tree, len_snippet=16)
    assert len(clips) == 8 and len({c.video for c in clips}) == 4
    img, sal = per_clip(clips, av=False)
    runs = {}
    for name, kw in (("device", {}), ("host", dict(decode="host")), ("one", dict(steps_per_load=1)), ("three", dict(steps_per_load=3))):
        runs[name] = train.load_batches(clips, ORDER, SIZE, device=DEV, **kw)
    for name, steps in runs.items():
        assert len(steps) == 3
        for b, at in zip(steps, ORDER):
            assert sorted(b) == ["img", "salmap", "sample_ids"] and b["sample_ids"] == at, name
            assert tuple(b["img"].shape) == (2, 3, 16) + SIZE and tuple(b["salmap"].shape) == (2, 1) + SIZE
            assert torch.equal(b["img"], img[at]) and torch.equal(b["salmap"], sal[at]), name


def test_load_batches_on_jpeg_files_with_audio(av_tree):
    from diff_sal_amd import audio_input, predict

    clips = train.list_av_train_clips(*av_tree, step_duration=20)          # step 4: windows from 1, 5, ..., 21
    assert len(clips) == 24 and len({c.video for c in clips}) == 4
    kept, removed = train.drop_empty_maps(clips, SIZE, device=DEV)
    assert [(c.video, c.gt_index) for c in removed] == [("V2", 15)] and len(kept) == 23
    assert kept == [c for c in clips if (c.video, c.gt_index) != ("V2", 15)]
    assert train.drop_empty_maps(clips, SIZE, device=DEV, decode="host", files_per_call=5)[1] == removed
    order = [[0, 22], [7, 13], [18, 4]]
    want = [kept[i] for s in order for i in s]
    img, sal = per_clip(want, av=True)
    audio = []
    for c in want:
        samples, rate = predict.read_wav(c.wav_file)
        starts, ends = audio_input.excerpt_table(c.n_frames, c.fps, rate, samples.shape[0])
        audio.append(audio_input.clip_audio(torch.from_numpy(samples).to(DEV), [int(starts[c.frame_indices[0]])],
                                            [int(ends[c.frame_indices[-1]])], size=(SIZE[0] // 2, SIZE[1] // 2)))
    audio = torch.cat(audio)
    for kw in ({}, dict(decode="host"), dict(steps_per_load=1), dict(steps_per_load=3)):
        steps = train.load_batches(kept, order, SIZE, device=DEV, **kw)
        for k, (b, at) in enumerate(zip(steps, order)):
            assert sorted(b) == ["audio", "img", "salmap", "sample_ids"] and b["sample_ids"] == at
            assert tuple(b["audio"].shape) == (2, 1, 9, SIZE[0] // 2, SIZE[1] // 2)
            assert torch.equal(b["img"], img[2 * k:2 * k + 2]) and torch.equal(b["salmap"], sal[2 * k:2 * k + 2]), kw
            assert torch.equal(b["audio"], audio[2 * k:2 * k + 2]), kw
    assert "audio" not in train.load_batches(kept, order[:1], SIZE, device=DEV, audio=False)[0]


def test_decode_groups(ucf_tree, av_tree):
    from diff_sal_amd import _image_files, jpeg, png

    clips = train.list_train_clips("ucf", ucf_tree, len_snippet=16)
    files = [clips[i].frame_files[k] for i, k in ((0, 0), (2, 1), (0, 2), (4, 3), (6, 4), (2, 5))]
    groups, where = png.decode_groups(_image_files.read_files(files), "RGB", DEV)
    assert where == [(0, 0), (1, 0), (0, 1), (2, 0), (3, 0), (1, 1)]                 # groups in order of first appearance
    assert [tuple(g.shape) for g in groups] == [(2,) + GEOMETRIES[0] + (3,), (2,) + GEOMETRIES[1] + (3,), (1,) + GEOMETRIES[2] + (3,),
                                                (1,) + GEOMETRIES[3] + (3,)]
    for f, (g, k) in zip(files, where):
        assert torch.equal(groups[g][k], pil([f], "RGB")[0])
    maps = [os.path.join(av_tree[2], v, "maps", "eyeMap_00003.jpg") for v in ("V3", "V1", "V3")]
    groups, where = jpeg.decode_groups(_image_files.read_files(maps), "L", DEV)
    assert where == [(0, 0), (1, 0), (0, 1)] and [tuple(g.shape) for g in groups] == [(2,) + GEOMETRIES[2], (1,) + GEOMETRIES[0]]
    for f, (g, k) in zip(maps, where):
        assert torch.equal(groups[g][k], pil([f], "L")[0])
    with pytest.raises(ValueError, match="file 1"):
        png.decode_groups([_image_files.read_files(files[:1])[0], b"not a png"], "RGB", DEV)
    with pytest.raises(ValueError, match="empty"):
        jpeg.decode_groups([], "RGB", DEV)
