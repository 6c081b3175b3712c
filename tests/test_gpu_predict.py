"""diff_sal_amd.predict on the device: the folder drivers against the same stages called by hand, file for file.  The arithmetic
is the same kernels on the same batches, so every comparison is equality.  Model at img_size (64, 128) with the closed-form
weights of the other GPU tests, DDIM with one step, device noise; frame files of 48 x 80 written here with Pillow."""
import os
import types
import wave

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import salunet_oracle as orc
from tests import _predict_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE = (64, 128)
FH, FW = 48, 80


def frame(seed, h=FH, w=FW):
    """a smooth pattern that moves with ``seed`` plus a little noise: uint8 [h, w, 3]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 100 * np.sin((x + 3 * seed) / 9.0 + c) * np.cos((y - 2 * seed) / 7.0 + 2 * c) for c in range(3)], -1)
    return np.clip(base + rng.integers(-12, 13, size=(h, w, 3)), 0, 255).astype(np.uint8)


def blob(seed, h=FH, w=FW):
    """an annotation-like map: one Gaussian blob that moves with ``seed``, uint8 [h, w]"""
    y, x = np.mgrid[0:h, 0:w]
    cy, cx = h * (0.3 + 0.05 * (seed % 7)), w * (0.2 + 0.07 * (seed % 9))
    return np.clip(255 * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * 6.0 ** 2)), 0, 255).astype(np.uint8)


def save(arr, path, **kw):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path, **kw)


def pil_frames(files, mode):
    return torch.from_numpy(np.stack([np.asarray(Image.open(f).convert(mode)) for f in files])).to(DEV)


@pytest.fixture(scope="module")
def nets():
    from diff_sal_amd.diff_model import VideoSaliencyModel
    from diff_sal_amd.sampling import DiffusionSampler
    from tests.test_gpu_encoders import build_audio, build_mvit
    from tests.test_gpu_salunet import build

    cfg = orc.SalUNetConfig(img_size=SIZE)
    dec = build(cfg, orc.synth_state_dict(orc.state_dict_template(cfg)))
    enc, _, _ = build_mvit("small")
    vgg, aan, _, _ = build_audio()
    visual = VideoSaliencyModel(channel_list=None, visual_net=enc, decoder_net=dec).to(DEV).eval()
    av = VideoSaliencyModel(channel_list=None, visual_net=enc, audio_net=vgg, spatiotemp_net=aan, decoder_net=dec).to(DEV).eval()
    kw = dict(sample_type="ddim", timesteps=1, noise_source="device", seed=11)
    return types.SimpleNamespace(visual=visual, av=av, s_visual=DiffusionSampler(visual, **kw), s_av=DiffusionSampler(av, **kw))


def hand_loop(sampler, clips, batch, loss_config=None):
    """The stages by hand for the clips of ONE video, in chunks of ``batch``: Pillow-loaded frames -> clip_rgb -> sample_image ->
    to_uint8.  Returns {gt_index: uint8 [h, w] on the host} and the per-chunk loss dictionaries (3-place rounded values)."""
    from diff_sal_amd import postprocess, predict, sal_losses, video_input

    files = sorted({f for c in clips for f in c.frame_files})
    frames = pil_frames(files, "RGB")
    out, losses = {}, []
    for lo in range(0, len(clips), batch):
        chunk = clips[lo:lo + batch]
        idx = [[files.index(f) for f in c.frame_files] for c in chunk]
        img = video_input.clip_rgb(frames, idx, size=SIZE, norm_value=255, mean=video_input.IMAGENET_MEAN, std=video_input.IMAGENET_STD)
        pred = sampler.sample_image(None, img=img, clip_ids=[predict.clip_id(c.video, c.gt_index) for c in chunk])
        u8 = postprocess.to_uint8(pred).cpu().numpy()
        for c, m in zip(chunk, u8):
            out[c.gt_index] = m
        if loss_config is not None:
            target = video_input.target_maps(pil_frames([c.gt_file for c in chunk], "L"), SIZE)
            d = sal_losses.get_kl_cc_sim_loss_wo_weight(loss_config, pred, target)
            losses.append({k: round(v.item(), 3) for k, v in d.items()})
    return out, losses


def read_back(paths):
    from diff_sal_amd import png

    return png.decode_files(paths, "L").cpu().numpy()


def expected_paths(out_root, want):
    return sorted(os.path.join(out_root, v, f"{g}.png") for v, gts in want.items() for g in gts)


def check_files(report, out_root, want, hand):
    """the files written are exactly ``want`` ({video: [gt_index]}) and each decodes to the hand loop's map"""
    found = sorted(os.path.join(d, f) for d, _, fs in os.walk(out_root) for f in fs)
    assert found == expected_paths(out_root, want) == sorted(report.files)
    assert report.clips == len(found) and report.skipped == []
    got = read_back(found)
    for path, m in zip(found, got):
        v, g = os.path.basename(os.path.dirname(path)), int(os.path.basename(path)[:-4])
        assert m.shape == SIZE and np.array_equal(m, hand[v][g]), (v, g, int((m != hand[v][g]).sum()))


LOSS_CFG = types.SimpleNamespace(loss=types.SimpleNamespace(loss_kl=True))
DHF1K_WANT = {"601": [9, 10, 11], "602": [9, 10, 11, 12, 13]}      # 19 frames: starts 0 .. 2; 21 frames: starts 0 .. 4; gt = start + 9


@pytest.fixture(scope="module")
def dhf1k(nets, tmp_path_factory):
    """the tree, and the hand loop's maps and losses with chunks of 3"""
    from diff_sal_amd import predict

    root = str(tmp_path_factory.mktemp("dhf1k"))
    for v, n in (("601", 19), ("602", 21)):
        for i in range(1, n + 1):
            save(frame(int(v) * 100 + i), os.path.join(root, "frames", v, f"{i}.png"))
            save(blob(int(v) + i), os.path.join(root, "maps", v, f"{i:04d}.png"))
    hand, losses = {}, []
    for v in ("601", "602"):
        hand[v], ls = hand_loop(nets.s_visual, predict.list_clips("dhf1k", root, len_snippet=16, videos=[v]), 3, LOSS_CFG)
        losses += ls
    return types.SimpleNamespace(root=root, hand=hand, losses=losses)


def test_dhf1k_files_are_the_hand_loops_maps(nets, dhf1k, tmp_path):
    from diff_sal_amd import predict

    out = str(tmp_path / "out")
    report = predict.predict_directory(nets.visual, nets.s_visual, "dhf1k", dhf1k.root, out, batch=3, size=SIZE, len_snippet=16)
    assert isinstance(report, predict.Report) and report.losses is None
    assert {v: sorted(gts) for v, gts in dhf1k.hand.items()} == DHF1K_WANT
    check_files(report, out, DHF1K_WANT, dhf1k.hand)
    assert not nets.visual.training


def test_predictions_do_not_depend_on_batch_or_video_order(nets, dhf1k, tmp_path):
    """device noise keyed by (video, gt_index) and the sampler's default clip_passes: the same pixels on any layout"""
    from diff_sal_amd import predict

    runs = {}
    for name, kw in (("b1", dict(batch=1)), ("b4", dict(batch=4)), ("reversed", dict(batch=4, videos=["602", "601"]))):
        out = str(tmp_path / name)
        rep = predict.predict_directory(nets.visual, nets.s_visual, "dhf1k", dhf1k.root, out, size=SIZE, len_snippet=16, **kw)
        assert sorted(rep.files) == expected_paths(out, DHF1K_WANT)
        runs[name] = read_back(expected_paths(out, DHF1K_WANT))
    assert [os.path.basename(os.path.dirname(f)) for f in rep.files][0] == "602"      # the reversed run did start with 602
    for name in ("b4", "reversed"):
        differ = (runs[name] != runs["b1"]).reshape(len(runs["b1"]), -1).sum(1)
        print(name, "pixels that differ from batch=1, per file:", differ.tolist())
        assert not differ.any(), (name, differ.tolist())


@pytest.mark.parametrize("data_type", ["ucf", "holly"])
def test_ucf_and_holly_trees(nets, tmp_path, data_type):
    from diff_sal_amd import predict

    root = str(tmp_path / "data")
    if data_type == "ucf":
        video, n = "Diving-Side-001", 18
        files = [f"Diving-Side_001_{i:03d}.png" for i in range(1, n + 1)]
        want = {video: [9, 10, 11]}                       # starts 0, 1 and the extra clip at 2; 1-based numbers
    else:
        video, n = "actioncliptest00001", 17
        files = [f"{video}_{i:05d}.png" for i in range(1, n + 1)]
        want = {video: [8, 9]}                            # start 0 and the extra clip at 1; 0-based positions
    for i, f in enumerate(files):
        save(frame(7000 + i), os.path.join(root, "testing", video, "images", f))
    clips = predict.list_clips(data_type, root, len_snippet=16)
    assert [(c.video, c.gt_index) for c in clips] == [(video, g) for g in want[video]]
    hand, _ = hand_loop(nets.s_visual, clips, 2)
    out = str(tmp_path / "out")
    report = predict.predict_directory(nets.visual, nets.s_visual, data_type, root, out, batch=2, size=SIZE, len_snippet=16)
    check_files(report, out, want, {video: hand})


def test_pillow_format_writes_the_same_pixels(nets, dhf1k, tmp_path):
    from diff_sal_amd import predict

    want = {"601": DHF1K_WANT["601"]}
    out = str(tmp_path / "pillow")
    report = predict.predict_directory(nets.visual, nets.s_visual, "dhf1k", dhf1k.root, out, batch=3, size=SIZE, len_snippet=16,
                                       videos=["601"], fmt="pillow")
    check_files(report, out, want, dhf1k.hand)
    for p in report.files:                                 # and Pillow reads its own files back to them too
        g = int(os.path.basename(p)[:-4])
        assert np.array_equal(np.asarray(Image.open(p)), dhf1k.hand["601"][g])
    with pytest.raises(ValueError, match="'jpg'"):
        predict.predict_directory(nets.visual, nets.s_visual, "dhf1k", dhf1k.root, out, size=SIZE, len_snippet=16, fmt="jpg")


def test_losses_are_the_meter_of_the_hand_loops_chunks(nets, dhf1k, tmp_path):
    """AverageMeterList: every chunk's value rounded to 3 places, every chunk weighed alike"""
    from diff_sal_amd import predict

    report = predict.predict_directory(nets.visual, nets.s_visual, "dhf1k", dhf1k.root, str(tmp_path / "out"), batch=3, size=SIZE,
                                       len_snippet=16, losses=True, loss_config=LOSS_CFG)
    assert len(dhf1k.losses) == 3 and report.chunks == 3      # 601: one chunk of 3; 602: chunks of 3 and 2
    assert set(report.losses) >= {"main", "cc", "sim", "nss", "total"}
    for k in ("main", "cc", "sim", "nss", "total"):
        total = 0.0
        for d in dhf1k.losses:
            total += d[k]
        print(k, report.losses[k], [d[k] for d in dhf1k.losses])
        assert report.losses[k] == total / 3 and np.isfinite(report.losses[k])
    assert report.losses["main"] != 0.0                        # loss_kl is on


def test_av_tree(nets, tmp_path):
    """one AVAD video: 20 JPEG frames of 64 x 48 at 25 fps, one second of 16 kHz mono int16 audio, eyeMap 11 all zero"""
    from diff_sal_amd import audio_input, jpeg, postprocess, predict, video_input

    name, n, fps, blank = "V1_Speech1", 20, 25, 11
    r = str(tmp_path)
    video_root, sal_root, audio_root = (os.path.join(r, d, "AVAD") for d in ("video_frames", "annotations", "video_audio"))
    for i in range(1, n + 1):
        save(frame(300 + i, 48, 64), os.path.join(video_root, name, f"img_{i:05d}.jpg"), quality=90)
        save(np.zeros((48, 64), np.uint8) if i == blank else blob(i, 48, 64), os.path.join(sal_root, name, "maps", f"eyeMap_{i:05d}.jpg"), quality=90)
    t = np.arange(16000)
    samples = (9000 * np.sin(2 * np.pi * 440 * t / 16000) + 3000 * np.sin(2 * np.pi * 1234 * t / 16000) * (t / 16000)).astype(np.int16)
    os.makedirs(os.path.join(audio_root, name))
    with wave.open(os.path.join(audio_root, name, name + ".wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(samples.astype("<i2").tobytes())
    fold = os.path.join(r, "fold.txt")
    with open(fold, "w") as f:
        f.write(f"{name} {n} {fps}\n")
    args = (video_root, fold, sal_root, audio_root)
    clips = predict.list_av_clips(*args)
    assert [(list(c.frame_indices), c.gt_index) for c in clips] == ref.av_exhaustive(n) and len(clips) == 19
    assert [c.gt_index for c in clips[:5]] == [9, 10, 11, 12, 13]
    kept = [c for c in clips if c.gt_index != blank]
    assert len(kept) == len(clips) - 1

    # the hand loop, with the driver's chunks of 4
    files = sorted({f for c in clips for f in c.frame_files})
    frames = pil_frames(files, "RGB")
    wav = torch.from_numpy(samples).to(DEV)
    starts, ends = audio_input.excerpt_table(n, float(fps), 16000, samples.shape[0])
    hand = {}
    for lo in range(0, len(kept), 4):
        chunk = kept[lo:lo + 4]
        img = video_input.clip_rgb(frames, [[files.index(f) for f in c.frame_files] for c in chunk], size=SIZE, pre_size=(240, 320),
                                   pre_filter="bicubic")
        audio = audio_input.clip_audio(wav, [int(starts[c.frame_indices[0]]) for c in chunk], [int(ends[c.frame_indices[-1]]) for c in chunk],
                                       size=(SIZE[0] // 2, SIZE[1] // 2))
        pred = nets.s_av.sample_image(None, img=img, audio=audio, clip_ids=[predict.clip_id(c.video_id, c.gt_index) for c in chunk])
        data, lengths = jpeg.encode(postprocess.to_uint8(pred))
        for c, row, ln in zip(chunk, data.cpu().numpy(), lengths.cpu().numpy()):
            hand[c.gt_index] = row[:int(ln)].tobytes()      # a later clip with the same median overwrites, as its file does

    out = str(tmp_path / "out")
    report = predict.predict_av(nets.av, nets.s_av, args, out, batch=4, size=SIZE)
    assert report.skipped == [(f"AVAD/{name}", blank, "its target map is all zero")]
    assert report.clips == len(kept) and len(report.files) == len(kept)
    found = sorted(os.path.join(d, f) for d, _, fs in os.walk(out) for f in fs)
    assert found == sorted(os.path.join(out, "avad", name, f"pred_sal_{g:06d}.jpg") for g in hand) == sorted(set(report.files))
    assert not os.path.exists(os.path.join(out, "avad", name, f"pred_sal_{blank:06d}.jpg"))
    for g, want in hand.items():
        with open(os.path.join(out, "avad", name, f"pred_sal_{g:06d}.jpg"), "rb") as f:
            assert f.read() == want, g
    # a list of clips is taken as well as the four paths; a set the reference has no folder name for is refused by name
    again = predict.predict_av(nets.av, nets.s_av, kept[:2], str(tmp_path / "again"), batch=4, size=SIZE, losses=True)
    assert again.clips == 2 and again.chunks == 1 and all(np.isfinite(v) for v in again.losses.values())
    import dataclasses
    with pytest.raises(ValueError, match="'Other'"):
        predict.predict_av(nets.av, nets.s_av, [dataclasses.replace(kept[0], video_id="Other/x")], out, size=SIZE)


def test_written_folder_scores_end_to_end(nets, dhf1k, tmp_path):
    """predict_directory's folder under a task folder is what evaluate.score_directory reads"""
    from diff_sal_amd import evaluate, predict

    pred_path = str(tmp_path / "preds")
    predict.predict_directory(nets.visual, nets.s_visual, "dhf1k", dhf1k.root, os.path.join(pred_path, "multi"), batch=4, size=SIZE,
                              len_snippet=16)
    gt_root = str(tmp_path / "gt")
    rng = np.random.default_rng(5)
    for v, gts in DHF1K_WANT.items():
        for g in gts:
            fix = np.zeros((72, 150), np.uint8)
            fix[rng.integers(0, 72, 12), rng.integers(0, 150, 12)] = 255
            save(blob(g, 72, 150), os.path.join(gt_root, "annotation", f"{int(v):04d}", "maps", f"{g:04d}.png"))
            save(fix, os.path.join(gt_root, "annotation", f"{int(v):04d}", "fixation", f"{g:04d}.png"))
    res = evaluate.score_directory(pred_path, gt_root, "dhf1k")
    assert list(res) == ["multi"] and set(res["multi"]) >= set(evaluate.DEFAULT_METRICS)
    assert all(np.isfinite(res["multi"][k]) for k in evaluate.DEFAULT_METRICS), res
    assert os.path.isfile(pred_path + "_metrics.csv")
