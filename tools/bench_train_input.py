#!/usr/bin/env python3
"""Times the training front end (``diff_sal_amd.train.load_batches``) on synthetic trees written here with Pillow, and the
grouped resize it rests on.

1. Grouped against per-geometry: ``video_input.transform_groups`` over the frames of a load against the same frames through one
   ``transform_frames`` call per geometry followed by the gather into batch order (what the code could do before the grouped
   call existed), at 1, 4 and 8 geometries, for the audio-visual chain (-> 240 x 320 bicubic -> 224 x 384 bilinear) and the
   visual one (-> 224 x 384 bilinear).  Both give the same bytes, which is asserted.
2. Data time per training step at batch 4 for ``decode="device"`` and ``decode="host"`` at ``steps_per_load`` 1, 4 and 8: an
   audio-visual-like tree (``img_%05d.jpg``, eight geometries between 240 x 320 and 480 x 720; no audio, to time the frames)
   and a DHF1K-like one (``'%d.png'``, 360 x 640).  Beside it: the step of a full-size ``VideoSaliencyModel`` (MViTv2-S + SalUNet
   at 224 x 384, random-init weights, ``DiffusionTrainStep`` with device noise) and a one-thread Pillow loader doing the
   reference's per-clip work (open, convert, resize(s), ToTensor, Normalize per frame of every clip, the map, stack, upload).
   The reference spreads that loader over DataLoader workers: divide by the workers you would give it.

The data times are the front end alone, synchronised at its end; in ``fit_directory`` the next load's file reads (and, with
``decode="host"``, its Pillow decode) run on host threads under the current steps.  Prints one JSON line.
usage: python tools/bench_train_input.py [--batch 4] [--steps 8] [--frames 40] [--no-step]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diff_sal_amd import train, video_input  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_train_input needs the GPU: a time taken elsewhere says nothing")
from PIL import Image  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--frames", type=int, default=40, help="frames per synthetic video")
ap.add_argument("--no-step", action="store_true", help="leave the full-size training step out")
args = ap.parse_args()
DEV, SIZE = "cuda", (224, 384)
GEOMETRIES = [(240, 320), (288, 352), (360, 480), (480, 640), (480, 720), (270, 480), (300, 400), (432, 576)]


def picture(seed, h, w):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([128 + 90 * np.sin((x + 3 * seed) / (40.0 + 9 * c)) * np.cos((y - 2 * seed) / (31.0 + 5 * c)) for c in range(3)], -1)
    return np.clip(base + rng.integers(-6, 7, size=(h, w, 3)), 0, 255).astype(np.uint8)


def blob(seed, h, w):
    y, x = np.mgrid[0:h, 0:w]
    return np.clip(255 * np.exp(-((y - h * 0.4) ** 2 + (x - w * (0.3 + 0.01 * (seed % 30))) ** 2) / (2 * 30.0 ** 2)), 0, 255).astype(np.uint8)


def save(a, path, **kw):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(a).save(path, **kw)


def write_av(root, n):
    lines = []
    for v, (h, w) in enumerate(GEOMETRIES):
        name = f"V{v + 1}"
        for i in range(1, n + 1):
            save(picture(100 * v + i, h, w), os.path.join(root, "video", "AVAD", name, f"img_{i:05d}.jpg"), quality=90)
            save(blob(v + i, h, w), os.path.join(root, "annot", "AVAD", name, "maps", f"eyeMap_{i:05d}.jpg"), quality=90)
        os.makedirs(os.path.join(root, "audio", "AVAD", name))
        open(os.path.join(root, "audio", "AVAD", name, name + ".wav"), "wb").close()      # listed, never read (audio=False)
        lines.append(f"{name} {n} 25.0")
    with open(os.path.join(root, "fold.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return train.list_av_train_clips(os.path.join(root, "video", "AVAD"), os.path.join(root, "fold.txt"), os.path.join(root, "annot", "AVAD"),
                                     os.path.join(root, "audio", "AVAD"), step_duration=20)


def write_dhf1k(root, n, videos=8):
    """``videos`` folders of ``2 * n`` frames of 360 x 640; the files of the first are written, the others are links to them (every
    path is still read and decoded on its own)"""
    for i in range(1, 2 * n + 1):
        save(picture(1000 + i, 360, 640), os.path.join(root, "frames", "1", f"{i}.png"))
        save(blob(i, 360, 640), os.path.join(root, "maps", "1", f"{i:04d}.png"))
    for v in range(2, videos + 1):
        for kind, name in (("frames", "{}.png"), ("maps", "{:04d}.png")):
            os.makedirs(os.path.join(root, kind, str(v)))
            for i in range(1, 2 * n + 1):
                os.link(os.path.join(root, kind, "1", name.format(i)), os.path.join(root, kind, str(v), name.format(i)))
    return train.list_train_clips("dhf1k", root, len_snippet=16)


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def grouped_against_per_geometry(frames_per_load):
    """ms of the resize chain over one load, its frames spread evenly over the first G geometries and interleaved in batch order"""
    rows = []
    rng = np.random.default_rng(5)
    for chain, pre in (("av", video_input.PRE_SIZE), ("visual", None)):
        for G in (1, 4, 8):
            per = frames_per_load // G
            groups = [torch.from_numpy(rng.integers(0, 256, size=(per, h, w, 3), dtype=np.uint8)).to(DEV) for h, w in GEOMETRIES[:G]]
            dst = [k * G + g for g in range(G) for k in range(per)]      # frame k of geometry g sits at k * G + g of the load
            dst_dev = torch.tensor(dst, device=DEV, dtype=torch.int32)

            def grouped():
                return video_input.transform_groups(groups, SIZE, pre_size=pre, dst=dst_dev if G > 1 else None)

            def per_geometry():
                parts = torch.cat([video_input.transform_frames(x, SIZE, pre_size=pre) for x in groups])
                if G == 1:
                    return parts
                out = torch.empty_like(parts)
                out[dst_dev.long()] = parts
                return out

            a, b = grouped(), per_geometry()      # warm-up: tables, allocator
            assert torch.equal(a, b), (chain, G)
            t_g, _ = timed(grouped, 10)
            t_p, _ = timed(per_geometry, 10)
            rows.append({"chain": chain, "geometries": G, "frames": per * G, "grouped_ms": 1e3 * t_g, "per_geometry_ms": 1e3 * t_p})
    return rows


def pillow_clip(c, av):
    """the reference's __getitem__ for one clip on the host: (float32 [3, 16, h, w], float32 [1, h, w])"""
    if av:
        mean, std, norm = video_input.DATASET_MEAN, video_input.DATASET_STD, video_input.DATASET_NORM_VALUE
    else:
        mean, std, norm = video_input.IMAGENET_MEAN, video_input.IMAGENET_STD, 255
    mean, std = (torch.tensor(v).view(3, 1, 1) for v in (mean, std))
    out = []
    for f in c.frame_files:
        img = Image.open(f).convert("RGB")
        if av:
            img = img.resize((video_input.PRE_SIZE[1], video_input.PRE_SIZE[0]))      # pil_loader: the default filter, bicubic
        img = img.resize((SIZE[1], SIZE[0]), Image.BILINEAR)
        out.append(torch.from_numpy(np.array(img)).permute(2, 0, 1).float().div(norm).sub_(mean).div_(std))
    gt = Image.open(c.gt_file).convert("L").resize((SIZE[1], SIZE[0]), Image.BILINEAR)
    return torch.stack(out, 0).permute(1, 0, 2, 3), torch.from_numpy(np.array(gt)).float().div(255)[None]


def data_times(clips, av):
    order = train.epoch_order(len(clips), 0, 0, 0, 1, args.batch)[:args.steps]
    assert len(order) == args.steps, (len(clips), args.steps)
    rows, first = [], None
    for decode in ("device", "host"):
        for per in (1, 4, 8):
            kw = dict(device=DEV, decode=decode, steps_per_load=per, audio=False)
            train.load_batches(clips, order[:per], SIZE, **kw)      # warm-up: tables, allocator
            t, out = timed(lambda: train.load_batches(clips, order, SIZE, **kw))
            if first is None:
                first = out
            assert all(torch.equal(a["img"], b["img"]) and torch.equal(a["salmap"], b["salmap"]) for a, b in zip(first, out))
            rows.append({"decode": decode, "steps_per_load": per, "data_ms_per_step": 1e3 * t / args.steps})
    geometries = len({Image.open(c.frame_files[0]).size for s in order for c in (clips[i] for i in s)})

    def pillow():
        for s in order[:2]:
            pairs = [pillow_clip(clips[i], av) for i in s]
            torch.stack([p[0] for p in pairs]).to(DEV), torch.stack([p[1] for p in pairs]).to(DEV)

    t_pil, _ = timed(pillow)
    return {"steps": args.steps, "batch": args.batch, "geometries_in_the_steps": geometries, "loads": rows,
            "pillow_one_thread_ms_per_step": 1e3 * t_pil / 2}


def step_time():
    from bench import Config, build_net
    from diff_sal_amd.diff_model import VideoSaliencyModel
    from diff_sal_amd.mvit import MViT
    from diff_sal_amd.train_step import DiffusionTrainStep

    net, _ = build_net(Config, DEV)
    enc = MViT(arch="small", out_scales=[0, 1, 2, 3]).to(DEV)
    model = VideoSaliencyModel(channel_list=None, visual_net=enc, decoder_net=net).to(DEV)
    trainer = DiffusionTrainStep(model, noise_source="device", seed=1)
    g = torch.Generator(device=DEV).manual_seed(3)
    img = torch.randn((args.batch, 3, 16) + SIZE, device=DEV, generator=g)
    sal = torch.rand((args.batch, 1) + SIZE, device=DEV, generator=g)
    for k in range(2):
        trainer.step(sal, {"img": img}, sample_ids=list(range(args.batch)))
    t, _ = timed(lambda: trainer.step(sal, {"img": img}, sample_ids=list(range(args.batch))), 3)
    return 1e3 * t


with tempfile.TemporaryDirectory() as tmp:
    result = {"size": list(SIZE), "resize": grouped_against_per_geometry(args.steps * args.batch * 16 // 2)}
    result["av_jpeg"] = data_times(write_av(os.path.join(tmp, "av"), args.frames), True)
    result["dhf1k_png"] = data_times(write_dhf1k(os.path.join(tmp, "dhf1k"), args.frames), False)
    if not args.no_step:
        result["train_step_ms"] = step_time()
    print(json.dumps(result))
