"""The listings of diff_sal_amd.predict (host code): trees of empty files against hand-worked lists and against the line-cited
restatement of the reference's dataset classes in tests/_predict_ref.py."""
import os
import wave

import numpy as np
import pytest

from diff_sal_amd import _image_files, predict, video_input
from tests import _predict_ref as ref


def touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def names(files):
    return [os.path.basename(f) for f in files]


def as_ref(clips):
    return [(c.video, names(c.frame_files), c.gt_index, os.path.basename(c.gt_file)) for c in clips]


def dhf1k_tree(root, videos):
    for v, n in videos.items():
        for i in range(1, n + 1):
            touch(os.path.join(root, "frames", v, f"{i}.png"))
    return str(root)


def split_tree(root, video, frame_names):
    for f in frame_names:
        touch(os.path.join(root, "testing", video, "images", f))
    os.makedirs(os.path.join(root, "testing", video, "maps"), exist_ok=True)
    return str(root)


def test_dhf1k_listing_is_the_hand_worked_one(tmp_path):
    root = dhf1k_tree(tmp_path, {"601": 20, "602": 16, "7": 40, "701": 40})
    clips = predict.list_clips("dhf1k", root, len_snippet=16)
    assert [c.video for c in clips] == ["601"] * 4                       # 602 has exactly 16 frames: no clip; 7 and 701 are not validation videos
    for start, c in enumerate(clips):
        assert len(c.frame_files) == 16
        assert list(c.frame_files) == [os.path.join(root, "frames", "601", f"{start + i + 1}.png") for i in range(16)]
    assert names(clips[0].frame_files)[0] == "1.png" and names(clips[0].frame_files)[-1] == "16.png"
    assert names(clips[3].frame_files)[0] == "4.png" and names(clips[3].frame_files)[-1] == "19.png"
    assert [c.gt_index for c in clips] == [9, 10, 11, 12]
    assert [c.gt_file for c in clips] == [os.path.join(root, "maps", "601", f"{g:04d}.png") for g in (9, 10, 11, 12)]
    assert as_ref(clips) == ref.dhf1k_val(root, 16)
    # the default len_snippet is the reference configuration's 32: none of these videos is longer
    assert predict.list_clips("dhf1k", root, videos=["601", "602"]) == []


def test_dhf1k_long_snippet_reads_16_frames_and_shortens_the_starts(tmp_path):
    root = dhf1k_tree(tmp_path, {"650": 40, "1000": 3, "99": 50})
    clips = predict.list_clips("dhf1k", root, len_snippet=32)
    assert [names(c.frame_files)[0] for c in clips] == [f"{s + 1}.png" for s in range(8)]      # starts 0 .. 7
    assert all(len(c.frame_files) == 16 and c.video == "650" for c in clips)
    assert [c.gt_index for c in clips] == list(range(9, 17))
    assert as_ref(clips) == ref.dhf1k_val(root, 32)
    # alternate 2, len_snippet 16: starts range(0, 40 - 32), every second frame
    alt = predict.list_clips("dhf1k", root, len_snippet=16, alternate=2)
    assert len(alt) == 8 and names(alt[1].frame_files) == [f"{2 + 2 * i}.png" for i in range(16)] and alt[1].gt_index == 18
    assert as_ref(alt) == ref.dhf1k_val(root, 16, alternate=2)
    # videos= replaces the list and its order, integer order otherwise
    both = predict.list_clips("dhf1k", root, len_snippet=32, videos=["99", 650])
    assert [c.video for c in both] == ["99"] * 18 + ["650"] * 8


def test_ucf_listing_takes_the_name_apart_at_its_last_hyphen(tmp_path):
    root = split_tree(tmp_path, "Diving-Side-001", [f"Diving-Side_001_{i:03d}.png" for i in range(1, 19)])
    split_tree(tmp_path, "Run-Side-010", [f"Run-Side_010_{i:03d}.png" for i in range(1, 13)])      # 12 frames: skipped
    clips = predict.list_clips("ucf", root, len_snippet=16)
    assert [c.video for c in clips] == ["Diving-Side-001"] * 3
    for start, c in zip((0, 1, 2), clips):                                # starts 0, 1 and the extra clip at 18 - 16
        assert names(c.frame_files) == ["Diving-Side_001_%03d.png" % (start + i + 1) for i in range(16)]
        assert os.path.dirname(c.frame_files[0]) == os.path.join(root, "testing", "Diving-Side-001", "images")
    assert [c.gt_index for c in clips] == [9, 10, 11]
    assert [c.gt_file for c in clips] == [os.path.join(root, "testing", "Diving-Side-001", "maps", "Diving-Side_001_%03d.png" % g)
                                          for g in (9, 10, 11)]
    assert as_ref(clips) == ref.ucf_test(root, 16)
    # where str.strip would eat into the name: "Golf-Swing-Back-001".strip("-001") is fine, "10-Run-001".strip("-001") is "Run"
    split_tree(tmp_path, "10-Run-001", [f"10-Run_001_{i:03d}.png" for i in range(1, 17)])
    only = predict.list_clips("ucf", root, len_snippet=16, videos=["10-Run-001"])
    assert len(only) == 1 and names(only[0].frame_files)[0] == "10-Run_001_001.png"
    with pytest.raises(ValueError, match="'nohyphen'"):
        split_tree(tmp_path, "nohyphen", [f"x_{i:03d}.png" for i in range(16)])
        predict.list_clips("ucf", root, len_snippet=16, videos=["nohyphen"])


def test_holly_listing_uses_positions_in_the_sorted_folder(tmp_path):
    frames17 = [f"actioncliptest00001_{i:05d}.png" for i in range(3, 20)]      # numbering that does not start at 0 or 1
    root = split_tree(tmp_path, "actioncliptest00001", frames17)
    split_tree(tmp_path, "actioncliptest00002", [f"actioncliptest00002_{i:05d}.png" for i in range(1, 13)])      # 12 frames: skipped
    clips = predict.list_clips("holly", root, len_snippet=16)
    assert [c.video for c in clips] == ["actioncliptest00001"] * 2
    assert names(clips[0].frame_files) == frames17[0:16] and names(clips[1].frame_files) == frames17[1:17]      # start 0, extra clip at 17 - 16
    assert [c.gt_index for c in clips] == [8, 9]                          # 0-based positions, not file numbers
    assert [c.gt_file for c in clips] == [os.path.join(root, "testing", "actioncliptest00001", "maps", frames17[g]) for g in (8, 9)]
    assert as_ref(clips) == ref.holly_test(root, 16)


def test_listing_refuses_what_the_model_cannot_serve(tmp_path):
    root = dhf1k_tree(tmp_path, {"601": 20})
    with pytest.raises(ValueError, match="gt_length=2"):
        predict.list_clips("dhf1k", root, len_snippet=16, gt_length=2)
    with pytest.raises(ValueError, match="'dhf2k'"):
        predict.list_clips("dhf2k", root)


def write_wav(path, channels=1, width=2, rate=16000, n=1600):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(bytes(n * channels * width))


def av_tree(root, videos):
    """``videos``: {name: (frames in the fold list, wav or not)} under the set AVAD"""
    lines = []
    for name, (n, wav) in videos.items():
        for i in range(1, n + 1):
            touch(os.path.join(root, "video_frames", "AVAD", name, f"img_{i:05d}.jpg"))
        os.makedirs(os.path.join(root, "annotations", "AVAD", name, "maps"), exist_ok=True)
        if wav:
            write_wav(os.path.join(root, "video_audio", "AVAD", name, name + ".wav"))
        lines.append(f"{name} {n} 25")
    fold = os.path.join(root, "fold.txt")
    with open(fold, "w") as f:
        f.write("\n".join(lines + ["V_missing 30 25"]) + "\n")      # no frame folder: skipped
    r = str(root)
    return (os.path.join(r, "video_frames", "AVAD") + "/", fold, os.path.join(r, "annotations", "AVAD"), os.path.join(r, "video_audio", "AVAD"))


def test_av_listing_pads_by_looping_and_labels_with_the_median(tmp_path):
    args = av_tree(tmp_path, {"V1_Speech1": (5, True), "V2_nowav": (9, False), "V3_one": (1, True)})
    clips = predict.list_av_clips(*args)
    assert [c.video for c in clips] == ["V1_Speech1"] * 4                  # j = 1 .. 4; no .wav and n_frames <= 1 drop a video
    assert [list(c.frame_indices) for c in clips] == [
        [1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 1],
        [2, 3, 4, 5, 2, 3, 4, 5, 2, 3, 4, 5, 2, 3, 4, 5],
        [3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4, 5, 3],
        [4, 5, 4, 5, 4, 5, 4, 5, 4, 5, 4, 5, 4, 5, 4, 5]]
    assert [c.gt_index for c in clips] == [3, 4, 4, 5]                     # 3.5 and 4.5 round half up
    assert [c.gt_index for c in clips] == [video_input.median_index(c.frame_indices) for c in clips]
    assert [(list(c.frame_indices), c.gt_index) for c in clips] == ref.av_exhaustive(5)
    c = clips[1]
    frames = os.path.join(str(tmp_path), "video_frames", "AVAD", "V1_Speech1")
    assert list(c.frame_files) == [os.path.join(frames, f"img_{i:05d}.jpg") for i in c.frame_indices]
    assert c.gt_file == os.path.join(str(tmp_path), "annotations", "AVAD", "V1_Speech1", "maps", "eyeMap_00004.jpg")
    assert c.wav_file == os.path.join(str(tmp_path), "video_audio", "AVAD", "V1_Speech1", "V1_Speech1.wav")
    assert c.video_id == "AVAD/V1_Speech1" and c.n_frames == 5 and c.fps == 25.0
    # a video of 20 frames: the first clips are whole, the last ones loop
    long = ref.av_exhaustive(20)
    assert long[0] == (list(range(1, 17)), 9) and long[4] == (list(range(5, 21)), 13) and len(long) == 19


def test_read_wav_takes_16_bit_mono_and_names_what_it_refuses(tmp_path):
    good = tmp_path / "a" / "good.wav"
    write_wav(good, rate=22050, n=300)
    samples, rate = predict.read_wav(str(good))
    assert samples.dtype == np.int16 and samples.shape == (300,) and rate == 22050
    stereo, eight, junk = tmp_path / "a" / "stereo.wav", tmp_path / "a" / "eight.wav", tmp_path / "a" / "junk.wav"
    write_wav(stereo, channels=2)
    write_wav(eight, width=1)
    junk.write_bytes(b"not a wave file at all")
    with pytest.raises(ValueError, match=r"stereo\.wav: 2 channels"):
        predict.read_wav(str(stereo))
    with pytest.raises(ValueError, match=r"eight\.wav: 8-bit"):
        predict.read_wav(str(eight))
    with pytest.raises(ValueError, match=r"junk\.wav: not a PCM"):
        predict.read_wav(str(junk))


def test_clip_ids_are_a_function_of_video_and_index_alone():
    a = predict.clip_id("601", 9)
    assert a == predict.clip_id(601, 9) and a != predict.clip_id("601", 10) and a != predict.clip_id("602", 9)
    assert 0 <= predict.clip_id("AVAD/V1_Speech1", 2 ** 31 - 1) < 2 ** 63
    with pytest.raises(ValueError, match="gt_index"):
        predict.clip_id("601", -1)


def test_read_files_keeps_the_order_on_any_thread_count(tmp_path):
    paths = []
    for i in range(40):
        p = tmp_path / f"{i}.bin"
        p.write_bytes(bytes([i]) * (i + 1))
        paths.append(str(p))
    want = [bytes([i]) * (i + 1) for i in range(40)]
    assert _image_files.read_files(paths) == want
    assert _image_files.read_files(paths, threads=16) == want
    assert _image_files.read_files(paths, threads=1000) == want and _image_files.MAX_READ_THREADS == 16
    assert _image_files.read_files([], threads=16) == []


def test_drivers_refuse_a_cpu_model(tmp_path):
    import torch

    from diff_sal_amd.sampling import DiffusionSampler

    class Top(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.decoder_net = torch.nn.Linear(2, 2)

    m = Top()
    s = DiffusionSampler(m)
    with pytest.raises(RuntimeError, match="GPU only"):
        predict.predict_directory(m, s, "dhf1k", str(tmp_path), str(tmp_path / "out"))
    with pytest.raises(RuntimeError, match="GPU only"):
        predict.predict_av(m, s, [], str(tmp_path / "out"))


def test_sample_image_runs_the_encoders_one_clip_per_pass_under_clip_passes():
    """what makes the drivers' files independent of ``batch``: with clip_passes the encoders see one clip at a time"""
    import torch

    from diff_sal_amd.sampling import DiffusionSampler

    seen = []

    def visual(img):
        seen.append(img.shape[0])
        return [img.mean(dim=(1, 2), keepdim=False)[:, None], img.amax(dim=(1, 2))[:, None]]

    def net(x, t, feats, a=None):
        return torch.sigmoid(0.5 * x + feats[0] - feats[1])

    top = type("M", (), {"decoder_net": staticmethod(net), "visual_net": staticmethod(visual)})()
    img, x = torch.randn(3, 3, 2, 4, 6), torch.randn(3, 1, 4, 6)
    outs = {}
    for passes in (False, True):
        seen.clear()
        s = DiffusionSampler(top, timesteps=1, sample_type="ddim", clip_passes=passes)
        outs[passes] = s.sample_image(x.clone(), img=img)
        assert seen == ([1, 1, 1] if passes else [3])
    assert torch.equal(outs[True], outs[False]) and outs[True].shape == x.shape


def test_videos_are_sharded_and_loss_sums_reduced_over_a_group(tmp_path):
    """the group= plumbing on a one-rank gloo group: shard_range of the videos, all-reduced sums and count"""
    import torch
    import torch.distributed as td

    created = not td.is_initialized()
    if created:
        td.init_process_group("gloo", store=td.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    assert td.get_world_size() == 1
    try:
        group = td.group.WORLD
        items = [("a", [1]), ("b", [2]), ("c", [3])]
        assert predict._shard(items, group) == items and predict._shard(items, None) == items
        meter = predict._Meter()
        for v in (0.1234, 0.5678):
            meter.update({k: torch.tensor(v) for k in predict.LOSS_NAMES})
        means, n = meter.means(torch.device("cpu"), group)
        assert n == 2 and means == {k: (0.123 + 0.568) / 2 for k in predict.LOSS_NAMES}
        assert predict._Meter().means(torch.device("cpu"), None)[1] == 0
    finally:
        if created:
            td.destroy_process_group()
