"""diff_sal_amd.train on the device: the folder drivers against a hand loop over the same stages.  The arithmetic is the same
kernels on the same batches in the same order, and with ``noise_source="device"`` every random input is a pure function of
(seed, step, sample id), so every comparison is equality.  Model, closed-form weights and the (64, 128) size are those of
tests/test_gpu_predict.py; the trees are those of tests/test_gpu_train_input.py (four videos, four geometries)."""
import csv
import os
import types

import pytest
import torch

from oracle import salunet_oracle as orc
from tests.test_gpu_train_input import write_av_tree, write_ucf_tree

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZE = (64, 128)
LOSS_CFG = types.SimpleNamespace(loss=types.SimpleNamespace(loss_kl=True))
UCF3 = ["Act-001", "Act-002", "Act-003"]      # six clips: three steps at batch 2


def make(av=False, lr=1e-3):
    """a fresh model with the closed-form weights and a DiffusionTrainStep with device noise around it"""
    from diff_sal_amd.diff_model import VideoSaliencyModel
    from diff_sal_amd.train_step import DiffusionTrainStep
    from tests.test_gpu_encoders import build_audio, build_mvit
    from tests.test_gpu_salunet import build

    torch.manual_seed(0)      # the audio-visual model's unused ``fc`` head (kept for its state_dict) is initialised from torch's generator
    cfg = orc.SalUNetConfig(img_size=SIZE)
    dec = build(cfg, orc.synth_state_dict(orc.state_dict_template(cfg)))
    enc, _, _ = build_mvit("small")
    enc.requires_grad_(True)
    if av:
        vgg, aan, _, _ = build_audio()
        model = VideoSaliencyModel(channel_list=None, visual_net=enc, audio_net=vgg, spatiotemp_net=aan, decoder_net=dec).to(DEV)
    else:
        model = VideoSaliencyModel(channel_list=None, visual_net=enc, decoder_net=dec).to(DEV)
    return model, DiffusionTrainStep(model, lr=lr, noise_source="device", seed=5)


def hand_loop(model, trainer, clips, epochs, batch, seed, run_epochs=None):
    """load_batches and trainer.step in epoch_order's order, the scheduler stepped once per epoch"""
    from torch.optim.lr_scheduler import MultiStepLR

    from diff_sal_amd import train

    sched = MultiStepLR(trainer.optimizer, train.milestones(epochs), 0.1)
    lrs = []
    for epoch in range(epochs if run_epochs is None else run_epochs):
        order = train.epoch_order(len(clips), epoch, seed, 0, 1, batch)
        for b in train.load_batches(clips, order, SIZE, device=DEV, audio=getattr(model, "audio_net", None) is not None):
            cond = {k: b[k] for k in ("img", "audio") if k in b}
            trainer.step(b["salmap"], cond, sample_ids=b["sample_ids"])
            lrs.append(trainer.lr)
        sched.step()
    return lrs


def same_state(a, b):
    """parameters and both moments, bit for bit"""
    return (torch.equal(a.flat.flat_p, b.flat.flat_p) and torch.equal(a.flat.exp_avg, b.flat.exp_avg)
            and torch.equal(a.flat.exp_avg_sq, b.flat.exp_avg_sq) and a.step_count == b.step_count)


def rows(path):
    return list(csv.reader(open(path), delimiter="\t"))


@pytest.fixture(scope="module")
def ucf(tmp_path_factory):
    return write_ucf_tree(str(tmp_path_factory.mktemp("ucf")))


@pytest.fixture(scope="module")
def fitted(ucf, tmp_path_factory):
    """fit_directory for two epochs of three steps at batch 2, uninterrupted"""
    from diff_sal_amd import train

    out = str(tmp_path_factory.mktemp("fit"))
    model, trainer = make()
    before = trainer.flat.flat_p.clone()
    report = train.fit_directory(model, trainer, "ucf", ucf, out, 2, 2, size=SIZE, seed=3, videos=UCF3, len_snippet=16, steps_per_load=2)
    assert not torch.equal(before, trainer.flat.flat_p)
    return types.SimpleNamespace(model=model, trainer=trainer, report=report, out=out)


def test_fit_directory_is_the_hand_loop(ucf, fitted):
    from diff_sal_amd import train

    clips = train.list_train_clips("ucf", ucf, len_snippet=16, videos=UCF3)
    assert len(clips) == 6
    model, trainer = make()
    lrs = hand_loop(model, trainer, clips, 2, 2, 3)
    assert lrs == [1e-3] * 3 + [trainer.lr] * 3 and trainer.step_count == 6
    assert same_state(fitted.trainer, trainer)
    for (k, a), (_, b) in zip(sorted(fitted.model.state_dict().items()), sorted(model.state_dict().items())):
        assert torch.equal(a, b), k                                       # BatchNorm's running statistics included
    r = fitted.report
    assert r.epochs == [1, 2] and r.step == 6 and r.best_epochs == [] and r.val_rows == [] and r.removed == []
    assert r.checkpoints == [os.path.join(fitted.out, "ckpt_1.pth"), os.path.join(fitted.out, "ckpt_2.pth")]
    log = rows(os.path.join(fitted.out, "train.log"))
    assert log[0] == list(train.TRAIN_HEADER) and [row[:2] for row in log[1:]] == [["1", "3"], ["2", "6"]]
    assert [float(row[-1]) for row in log[1:]] == [1e-3, lrs[-1]]
    assert all(float(v) == round(float(v), 3) for row in log[1:] for v in row[2:7])
    assert float(log[1][2]) == float(log[1][3]) > 0                       # the built-in MSE counts as main and total
    assert rows(os.path.join(fitted.out, "val.log")) == [list(train.VAL_HEADER)]
    assert not os.path.exists(os.path.join(fitted.out, "best.pth"))


def test_steps_per_load_decode_and_prefetch_do_not_change_the_run(ucf, fitted, tmp_path):
    from diff_sal_amd import train

    model, trainer = make()
    train.fit_directory(model, trainer, "ucf", ucf, str(tmp_path), 2, 2, size=SIZE, seed=3, videos=UCF3, len_snippet=16, steps_per_load=3,
                        decode="device", prefetch=False)
    assert same_state(fitted.trainer, trainer)


def test_resume_gives_the_uninterrupted_run(ucf, fitted, tmp_path):
    from diff_sal_amd import train

    kw = dict(size=SIZE, seed=3, videos=UCF3, len_snippet=16, steps_per_load=2)
    model, trainer = make()
    first = train.fit_directory(model, trainer, "ucf", ucf, str(tmp_path), 2, 2, stop_epoch=1, **kw)
    assert first.epochs == [1] and first.step == 3 and os.listdir(str(tmp_path)).count("ckpt_1.pth") == 1
    assert not same_state(fitted.trainer, trainer)
    model2, trainer2 = make()                                             # fresh objects
    second = train.fit_directory(model2, trainer2, "ucf", ucf, str(tmp_path), 2, 2, resume=os.path.join(str(tmp_path), "ckpt_1.pth"), **kw)
    assert second.epochs == [2] and second.step == 6
    assert same_state(fitted.trainer, trainer2)
    # the checkpoints of both runs agree, and load into the reference-format consumers the project has
    a = torch.load(os.path.join(fitted.out, "ckpt_2.pth"), map_location="cpu")
    b = torch.load(os.path.join(str(tmp_path), "ckpt_2.pth"), map_location="cpu")
    assert list(a) == ["state_dict", "optim_dict", "epoch", "step"] and (a["epoch"], a["step"]) == (b["epoch"], b["step"]) == (2, 6)
    assert all(torch.equal(a["state_dict"][k], b["state_dict"][k]) for k in a["state_dict"])
    model3, trainer3 = make()
    assert model3.load_state_dict(a["state_dict"], strict=True).missing_keys == []
    trainer3.load_state_dict(a["optim_dict"])
    assert same_state(fitted.trainer, trainer3) and trainer3.lr == fitted.trainer.lr
    plain = torch.optim.Adam(model3.parameters(), lr=1.0)                 # and into torch.optim.Adam, the reference's optimizer
    plain.load_state_dict(a["optim_dict"])
    assert plain.param_groups[0]["lr"] == fitted.trainer.lr


def test_learning_rate_follows_the_milestones(ucf, tmp_path, monkeypatch):
    from diff_sal_amd import ops, train

    seen = []
    real = ops.adam_step

    def spy(*a, **k):
        seen.append(k["lr"])
        return real(*a, **k)

    monkeypatch.setattr(ops, "adam_step", spy)
    model, trainer = make(lr=1e-3)
    report = train.fit_directory(model, trainer, "ucf", ucf, str(tmp_path), 4, 2, size=SIZE, seed=1, videos=UCF3[:1], len_snippet=16)
    assert report.step == 4 and train.milestones(4) == [2, 3]
    assert seen == [1e-3, 1e-3, 1e-3 * 0.1, 1e-3 * 0.1 * 0.1]             # what the fused clip + Adam kernel was given
    assert [float(r[-1]) for r in rows(os.path.join(str(tmp_path), "train.log"))[1:]] == seen


def test_validation_row_and_best(ucf, tmp_path):
    from diff_sal_amd import predict, train
    from diff_sal_amd.sampling import DiffusionSampler

    model, trainer = make()
    sampler = DiffusionSampler(model, sample_type="ddim", timesteps=1, noise_source="device", seed=11)
    out = str(tmp_path / "out")
    report = train.fit_directory(model, trainer, "ucf", ucf, out, 1, 2, size=SIZE, seed=3, videos=UCF3[:1], len_snippet=16, sampler=sampler,
                                 loss_config=LOSS_CFG, val_batch=2)
    after = predict.predict_directory(model, sampler, "ucf", ucf, str(tmp_path / "pred"), batch=2, size=SIZE, losses=True,
                                      loss_config=LOSS_CFG, len_snippet=16)
    assert after.chunks == 2 and after.clips == 3
    want = train.val_row(1, 1, after.losses)
    assert report.val_rows == [want]
    log = rows(os.path.join(out, "val.log"))
    assert log[0] == list(train.VAL_HEADER) and log[1] == [str(want[k]) for k in train.VAL_HEADER]
    assert sorted(f for _, _, fs in os.walk(out) for f in fs) == sorted(
        ["train.log", "val.log", "ckpt_1.pth"] + (["best.pth"] if after.losses["total"] > 0.0 else []))      # no prediction file
    assert report.best_epochs == ([1] if after.losses["total"] > 0.0 else [])


def test_fit_av_is_the_hand_loop(tmp_path):
    from diff_sal_amd import train

    sets = [write_av_tree(str(tmp_path / "av"), n_frames=24, zero=("V2", 13))]
    kw = dict(step_duration=28)                                          # step 12: windows from 1 and 13, labelled by frames 13 and 17
    model, trainer = make(av=True)
    out = str(tmp_path / "out")
    report = train.fit_av(model, trainer, sets, out, 2, 2, size=SIZE, seed=9, steps_per_load=2, **kw)
    assert [(c.video, c.gt_index) for c in report.removed] == [("V2", 13)] and report.step == 6 and report.epochs == [1, 2]
    clips = [c for c in train.list_av_train_clips(*sets[0], **kw) if (c.video, c.gt_index) != ("V2", 13)]
    assert len(clips) == 7
    model2, trainer2 = make(av=True)
    hand_loop(model2, trainer2, clips, 2, 2, 9)
    assert same_state(trainer, trainer2)
    assert [r[:2] for r in rows(os.path.join(out, "train.log"))[1:]] == [["1", "3"], ["2", "6"]]
