"""The host side of diff_sal_amd.train: the training listings on trees of empty files against the line-cited restatement of the
reference's dataset classes in tests/_train_ref.py, the epoch order against torch's DistributedSampler and DataLoader, and the
loop's bookkeeping (checkpoint dictionary, log rows, the best.pth rule, resume) without a GPU."""
import csv
import os

import pytest
import torch

from diff_sal_amd import train
from tests import _train_ref as ref


def touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, "wb").close()


def as_ref(clips):
    return [(c.video, [os.path.basename(f) for f in c.frame_files], c.gt_index, os.path.basename(c.gt_file)) for c in clips]


def dhf1k_tree(root, videos):
    for v, n in videos.items():
        for i in range(1, n + 1):
            touch(os.path.join(root, "frames", v, f"{i}.png"))
    return str(root)


def ucf_tree(root, videos):
    for v, n in videos.items():
        name, _, number = v.rpartition("-")
        for i in range(1, n + 1):
            touch(os.path.join(root, "training", v, "images", f"{name}_{number}_{i:03d}.png"))
        os.makedirs(os.path.join(root, "training", v, "maps"), exist_ok=True)
    touch(os.path.join(root, "testing", "Other-001", "images", "Other_001_001.png"))      # not a training video
    return str(root)


def holly_tree(root, videos):
    for v, n in videos.items():
        for i in range(n):
            touch(os.path.join(root, "training", v, "images", f"{v}_{3 * i + 2:05d}.png"))      # names that are not their positions
        os.makedirs(os.path.join(root, "training", v, "maps"), exist_ok=True)
    return str(root)


SNIPPETS = [(16, 1), (16, 2), (32, 1), (32, 2)]


@pytest.mark.parametrize("len_snippet,alternate", SNIPPETS)
def test_dhf1k_train_listing(tmp_path, len_snippet, alternate):
    exact = alternate * len_snippet
    root = dhf1k_tree(tmp_path, {"1": 100, "2": exact, "600": exact + 1, "601": 100, "12": exact + 17})
    clips = train.list_train_clips("dhf1k", root, len_snippet=len_snippet, alternate=alternate)
    assert as_ref(clips) == ref.dhf1k_train(root, len_snippet, alternate)
    assert [c.video for c in clips if c.video in ("2", "601")] == []      # exactly alternate * len_snippet frames: no clip; 601: validation
    assert sorted({int(c.video) for c in clips}) == [1, 12, 600]
    assert all(len(c.frame_files) == 16 for c in clips)                  # 16 frames whatever len_snippet says
    one = [c for c in clips if c.video == "1"]
    assert [int(os.path.basename(c.frame_files[0])[:-4]) - 1 for c in one] == list(range(0, 100 - exact, 16))      # skip_window 16
    assert one[0].gt_index == 1 + 8 * alternate and one[0].gt_file == os.path.join(root, "maps", "1", "%04d.png" % one[0].gt_index)
    assert [c.video for c in clips if c.video == "12"] == ["12"] * 2     # starts 0 and 16 of range(0, 17, 16)


@pytest.mark.parametrize("len_snippet,alternate", SNIPPETS)
def test_ucf_train_listing(tmp_path, len_snippet, alternate):
    exact = alternate * len_snippet
    root = ucf_tree(tmp_path, {"Diving-Side-001": exact + 40, "Run-Side-010": exact, "Walk-Front-002": 5, "Kick-003": exact + 1})
    clips = train.list_train_clips("ucf", root, len_snippet=len_snippet, alternate=alternate)
    assert as_ref(clips) == ref.ucf_train(root, len_snippet, alternate)
    # a short video is not skipped, it gives no clip; neither does one of exactly alternate * len_snippet frames; no extra last clip
    assert [c.video for c in clips] == ["Diving-Side-001"] * 3 + ["Kick-003"]
    assert os.path.basename(clips[1].frame_files[0]) == "Diving-Side_001_017.png"
    assert clips[1].gt_index == 17 + 8 * alternate and os.path.basename(clips[1].gt_file) == "Diving-Side_001_%03d.png" % clips[1].gt_index
    assert os.path.dirname(clips[0].gt_file) == os.path.join(root, "training", "Diving-Side-001", "maps")


@pytest.mark.parametrize("len_snippet,alternate", SNIPPETS)
def test_holly_train_listing(tmp_path, len_snippet, alternate):
    exact = alternate * len_snippet
    root = holly_tree(tmp_path, {"actioncliptrain00002": exact + 33, "actioncliptrain00001": exact, "actioncliptrain00007": 3})
    clips = train.list_train_clips("holly", root, len_snippet=len_snippet, alternate=alternate)
    assert as_ref(clips) == ref.holly_train(root, len_snippet, alternate)
    assert [c.video for c in clips] == ["actioncliptrain00002"] * 3      # starts 0, 16, 32
    # 0-based positions in the sorted listing, for the frames and for the map
    names = sorted(os.listdir(os.path.join(root, "training", "actioncliptrain00002", "images")))
    assert [os.path.basename(f) for f in clips[2].frame_files] == [names[32 + alternate * i] for i in range(16)]
    assert clips[2].gt_index == 32 + 8 * alternate and os.path.basename(clips[2].gt_file) == names[clips[2].gt_index]


def test_list_train_clips_arguments(tmp_path):
    with pytest.raises(ValueError, match="data_type"):
        train.list_train_clips("avad", str(tmp_path))
    with pytest.raises(ValueError, match="at least 1"):
        train.list_train_clips("ucf", str(tmp_path), len_snippet=0)
    assert train.skip_window(8) == 8 and train.skip_window(16) == 16 and train.skip_window(17) == 16 and train.skip_window(48) == 16


def av_tree(root, videos):
    lines = []
    for name, n in videos.items():
        os.makedirs(os.path.join(root, "video", "AVAD", name), exist_ok=True)
        os.makedirs(os.path.join(root, "annot", "AVAD", name, "maps"), exist_ok=True)
        touch(os.path.join(root, "audio", "AVAD", name, name + ".wav"))
        lines.append(f"{name} {n} 25.0")
    lines.append("V_missing 100 25.0")                 # no folder: skipped
    fold = os.path.join(root, "fold.txt")
    with open(fold, "w") as f:
        f.write("\n".join(lines) + "\n")
    return os.path.join(root, "video", "AVAD"), fold, os.path.join(root, "annot", "AVAD"), os.path.join(root, "audio", "AVAD")


AV_FRAMES = (2, 17, 75, 76, 90, 91, 200)


def test_av_train_listing(tmp_path):
    videos = {f"V{n:03d}": n for n in AV_FRAMES}
    videos["V001"] = 1                                  # n_frames <= 1: skipped
    args = av_tree(str(tmp_path), videos)
    clips = train.list_av_train_clips(*args)
    assert {c.video for c in clips} == {f"V{n:03d}" for n in AV_FRAMES}
    for n in AV_FRAMES:
        mine = [c for c in clips if c.video == f"V{n:03d}"]
        want = ref.av_train(n)
        assert [(list(c.frame_indices), c.gt_index) for c in mine] == want, n
        for c in mine:
            assert c.video_id == f"AVAD/V{n:03d}" and c.n_frames == n and c.fps == 25.0 and len(c.frame_files) == 16
            assert [os.path.basename(f) for f in c.frame_files] == ["img_%05d.jpg" % i for i in c.frame_indices]
            assert c.gt_file == os.path.join(args[2], c.video, "maps", "eyeMap_%05d.jpg" % c.gt_index)
            assert c.wav_file == os.path.join(args[3], c.video, c.video + ".wav")
    by = {n: [c for c in clips if c.video == f"V{n:03d}"] for n in AV_FRAMES}
    # step = 90 - 16 = 74: windows start at 1, 75, 149
    assert [len(by[n]) for n in AV_FRAMES] == [1, 1, 1, 2, 2, 2, 3]
    assert by[2][0].frame_indices == (1, 2) * 8 and by[2][0].gt_index == 2              # the cycle padding; median 1.5 rounds half up
    assert by[17][0].frame_indices == tuple(range(1, 17)) and by[17][0].gt_index == 9     # 17 frames, centre 8: indices 0 .. 15; median 8.5 -> 9
    # range(1, 75, 74) holds 1 alone: a 75-frame video has no second window, and no window of the rule has a single frame (j is
    # below n_frames, so frames j and j + 1 exist).  The shortest second window is that of 76 frames, which has two.
    assert by[75][0].frame_indices == tuple(range(30, 46)) and by[75][0].gt_index == 38   # window 1 .. 75, centre 37: 30 .. 45, median 37.5 -> 38
    assert by[76][1].frame_indices == (75, 76) * 8 and by[76][1].gt_index == 76
    assert by[90][0].frame_indices == tuple(range(38, 54)) and by[90][0].gt_index == 46  # window 1 .. 90, centre 45: 38 .. 53, median 45.5 -> 46
    assert by[91][1].frame_indices == tuple(range(75, 91)) and by[91][1].gt_index == 83  # window 75 .. 91 (17 frames), centre 8: its first 16
    assert by[200][2].frame_indices[0] == 149 + 26 - 8                                   # window 149 .. 200 (52 frames), centre 26
    # sample_duration and step_duration are the listing's parameters
    short = train.list_av_train_clips(*args, sample_duration=4, step_duration=10)
    assert [(list(c.frame_indices), c.gt_index) for c in short if c.video == "V017"] == ref.av_train(17, 4, 10)


def test_epoch_order_covers_every_index_once():
    for n, world, batch in ((23, 1, 4), (23, 2, 4), (23, 3, 2), (5, 3, 1), (2, 3, 1)):
        for epoch in (0, 1, 5):
            ranks = [train.epoch_order(n, epoch, 7, r, world, batch) for r in range(world)]
            per_rank = -(-n // world)
            assert all(len(b) == batch for r in ranks for b in r)
            assert all(len(r) == per_rank // batch for r in ranks)                       # incomplete batches are dropped
            # undo the drop: with batch 1 every index a rank owns shows
            full = [[i for b in train.epoch_order(n, epoch, 7, r, world, 1) for i in b] for r in range(world)]
            interleaved = [full[k % world][k // world] for k in range(per_rank * world)]
            assert sorted(interleaved[:n]) == list(range(n))                             # every index once, before the padding
            assert interleaved[n:] == (interleaved[:n] * world)[:per_rank * world - n]  # the padding walks the order again
            if per_rank * world == n:
                assert not set(full[0]) & set(full[-1]) or world == 1                    # ranks are disjoint
    assert train.epoch_order(23, 3, 7, 1, 2, 4) == train.epoch_order(23, 3, 7, 1, 2, 4)  # a pure function
    assert train.epoch_order(23, 3, 7, 1, 2, 4) != train.epoch_order(23, 4, 7, 1, 2, 4)  # reshuffled per epoch
    assert train.epoch_order(23, 3, 7, 0, 1, 4) == train.epoch_order(23, 0, 10, 0, 1, 4)  # seed + epoch seeds the generator
    with pytest.raises(ValueError):
        train.epoch_order(10, 0, 0, 2, 2, 1)
    with pytest.raises(ValueError):
        train.epoch_order(0, 0, 0, 0, 1, 1)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_epoch_order_is_the_distributed_sampler(world):
    from torch.utils.data import DataLoader, Dataset
    from torch.utils.data.distributed import DistributedSampler

    class Items(Dataset):
        def __init__(self, n):
            self.n = n

        def __len__(self):
            return self.n

        def __getitem__(self, i):
            return i

    for n, batch, seed in ((23, 4, 0), (24, 3, 5), (7, 2, 11), (2, 1, 3)):
        data = Items(n)
        for rank in range(world):
            sampler = DistributedSampler(data, num_replicas=world, rank=rank, shuffle=True, seed=seed)
            loader = DataLoader(data, batch_size=batch, drop_last=True, sampler=sampler)      # R/datasets/prepare_data.py:8-24
            for epoch in (0, 1, 4):
                sampler.set_epoch(epoch)
                assert [b.tolist() for b in loader] == train.epoch_order(n, epoch, seed, rank, world, batch), (n, rank, epoch)


class StubTrainer:
    """the checkpoint surface of DiffusionTrainStep: an Adam-format dictionary in, the same out"""

    def __init__(self, lr=1e-4, step=0):
        self.sd = {"state": {0: {"step": torch.tensor(float(step))}}, "param_groups": [{"lr": lr, "params": [0, 1]}]}

    def state_dict(self):
        return self.sd

    def load_state_dict(self, sd):
        self.sd = sd


def test_checkpoint_dictionary_and_resume(tmp_path):
    model = torch.nn.Linear(3, 2)
    trainer = StubTrainer(lr=2.5e-5, step=6)
    states = train.checkpoint(model, trainer, 2, 6)
    assert list(states) == ["state_dict", "optim_dict", "epoch", "step"]              # R/diffusion_trainer.py:408-413
    assert states["epoch"] == 2 and states["step"] == 6 and states["optim_dict"] is trainer.sd
    assert set(states["state_dict"]) == {"weight", "bias"}
    path = os.path.join(tmp_path, "ckpt_2.pth")
    torch.save(states, path)
    fresh_model, fresh_trainer = torch.nn.Linear(3, 2), StubTrainer()
    assert not torch.equal(fresh_model.weight, model.weight)
    assert train.resume_from(path, fresh_model, fresh_trainer) == (2, 6)              # epoch and step are restored
    assert torch.equal(fresh_model.weight, model.weight) and torch.equal(fresh_model.bias, model.bias)
    assert fresh_trainer.sd["param_groups"][0]["lr"] == 2.5e-5 and float(fresh_trainer.sd["state"][0]["step"]) == 6.0
    del states["step"]
    torch.save(states, path)
    with pytest.raises(ValueError, match="step"):
        train.resume_from(path, fresh_model, fresh_trainer)


def test_log_rows(tmp_path):
    means = {"total": 1.23456, "main": 0.0004, "cc": -0.5555, "sim": 0.3335, "nss": 2.0, "extra": 9}
    row = train.train_row(3, 120, means, 1e-5)
    # print_train_info, R/diffusion_trainer.py:977-988: round(avg, 3), the lr as it is
    assert row == {"epoch": 3, "total_step": 120, "loss": round(1.23456, 3), "main": round(0.0004, 3), "cc": round(-0.5555, 3),
                   "sim": round(0.3335, 3), "nss": 2.0, "lr": 1e-5}
    vrow = train.val_row(3, 120, means)
    assert list(vrow) == ["epoch", "total_step", "loss", "main", "cc", "sim", "nss"] and vrow["loss"] == 1.235
    path = os.path.join(tmp_path, "train.log")
    log = train.Logger(path, train.TRAIN_HEADER)
    log.log(row)
    log.log({"epoch": 4})                                                               # a missing column is written as 0.0
    log.close()
    rows = list(csv.reader(open(path), delimiter="\t"))
    assert rows[0] == ["epoch", "total_step", "loss", "main", "cc", "sim", "nss", "lr"]
    assert rows[1] == ["3", "120", "1.235", "0.0", "-0.555" if round(-0.5555, 3) == -0.555 else "-0.556", "0.334" if round(0.3335, 3) == 0.334 else "0.333", "2.0", "1e-05"]
    assert rows[2] == ["4"] + ["0.0"] * 7
    assert train.VAL_HEADER == train.TRAIN_HEADER[:-1]
    # a second run appends, header included, as the reference's Logger does
    train.Logger(path, train.TRAIN_HEADER).close()
    assert len(list(csv.reader(open(path), delimiter="\t"))) == 4


def test_device_meters_on_the_host():
    m = train.DeviceMeters("cpu")
    m.update({"total": torch.tensor(1.2344), "main": torch.tensor(0.5), "cc": 0.0, "sim": torch.tensor(0.25), "nss": torch.tensor(-1.0006)})
    m.update({"total": torch.tensor(2.0006), "main": torch.tensor(0.5), "cc": 0.0, "sim": torch.tensor(0.75), "nss": torch.tensor(1.0)})
    got = m.means()
    assert got == {"main": 0.5, "cc": 0.0, "sim": 0.5, "nss": (-1.001 + 1.0) / 2, "total": (1.234 + 2.001) / 2}


def test_best_rule_on_a_recorded_sequence():
    values = [-0.2, 0.0, 1.5, 1.5, 1.2, 1.7, 0.3, 2.0]
    keeper = train.BestKeeper()
    got = [epoch + 1 for epoch, v in enumerate(values) if keeper.is_best(v)]
    assert got == ref.best_epochs(values) == [3, 6, 8]       # larger wins, a tie does not, nothing at or below 0.0 ever does
    assert keeper.min_loss == 2.0
    assert [e for e, v in enumerate([-1.0, -0.5]) if train.BestKeeper().is_best(v)] == []


def test_milestones():
    assert train.milestones(4) == [2, 3] and train.milestones(2) == [1, 1] and train.milestones(10) == [5, 7]      # R/util/utils.py:120-121
    assert train.milestones(1) == [0, 0]


def test_front_end_arguments():
    with pytest.raises(ValueError, match="decode"):
        train.load_batches([object()], [[0]], (8, 8), decode="pillow")
    with pytest.raises(ValueError, match="outside the listing"):
        train.load_batches([object()], [[1]], (8, 8))
    with pytest.raises(RuntimeError, match="GPU only"):
        train.load_batches([object()], [[0]], (8, 8), device="cpu")
    with pytest.raises(RuntimeError, match="GPU only"):
        train.fit_directory(torch.nn.Linear(2, 2), StubTrainer(), "dhf1k", "/nonexistent", "/nonexistent", 1, 1, videos=[])
