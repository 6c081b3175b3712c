#!/usr/bin/env python3
"""Times ``predict.predict_directory`` on one synthetic DHF1K-like video (300 frames of 360 x 640, written here with Pillow) at
full model size (MViTv2-S + SalUNet at 224 x 384, random-init weights, DDIM), and beside it the same loop -- same model, same
sampler, same chunks, same export -- fed by a restatement of the reference's host loader on one thread: per clip and frame
``Image.open(f).convert('RGB')``, ``Resize((224, 384))``, ``ToTensor``, ``Normalize`` (R/datasets/meta_data.py:27-31,
R/datasets/dhf1k_data.py:76-81), stacked and uploaded per chunk.  The reference spreads that loader over DataLoader workers; one
thread is what one worker does, so divide by the workers you would give it.  One warm-up pass over the first clips, then one timed
pass of each loop over the whole video; a pass is tens of seconds, so it is timed once.  Prints one JSON line with both clips/s.
usage: python tools/bench_predict.py [--frames 300] [--batch 4] [--timesteps 1] [--len-snippet 32]"""
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
from bench import Config, build_net  # noqa: E402
from diff_sal_amd import png, predict, video_input  # noqa: E402
from diff_sal_amd.diff_model import VideoSaliencyModel  # noqa: E402
from diff_sal_amd.mvit import MViT  # noqa: E402
from diff_sal_amd.sampling import DiffusionSampler  # noqa: E402

if not torch.cuda.is_available():
    raise SystemExit("bench_predict needs the GPU: a time taken elsewhere says nothing")
from PIL import Image  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=300)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--timesteps", type=int, default=1)
ap.add_argument("--len-snippet", type=int, default=32)
args = ap.parse_args()
H, W, SIZE, DEV = 360, 640, (224, 384), "cuda"


def write_video(root, n):
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    texture = rng.integers(-18, 19, size=(H, W, 1)).astype(np.float32)
    os.makedirs(os.path.join(root, "frames", "601"))
    for t in range(n):
        base = np.stack([128 + 90 * np.sin((x + 3 * t) / (40.0 + 9 * c)) * np.cos((y - 2 * t) / (31.0 + 5 * c)) for c in range(3)], axis=-1)
        img = np.clip(base + texture + rng.integers(-4, 5, size=(H, W, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "frames", "601", f"{t + 1}.png"))


def host_clip(clip):
    """the reference's __getitem__ for one clip: float32 [3, 16, 224, 384] on the host"""
    mean, std = (torch.tensor(v).view(3, 1, 1) for v in (video_input.IMAGENET_MEAN, video_input.IMAGENET_STD))
    out = []
    for f in clip.frame_files:
        img = Image.open(f).convert("RGB").resize((SIZE[1], SIZE[0]), Image.BILINEAR)
        t = torch.from_numpy(np.array(img)).permute(2, 0, 1).float().div(255)
        out.append(t.sub_(mean).div_(std))
    return torch.stack(out, 0).permute(1, 0, 2, 3)


@torch.no_grad()
def host_loop(sampler, clips, out_root, batch):
    for lo in range(0, len(clips), batch):
        chunk = clips[lo:lo + batch]
        img = torch.stack([host_clip(c) for c in chunk]).to(DEV)
        pred = sampler.sample_image(None, img=img, clip_ids=[predict.clip_id(c.video, c.gt_index) for c in chunk])
        png.save_predictions(pred, [c.video for c in chunk], [c.gt_index for c in chunk], out_root)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


with tempfile.TemporaryDirectory() as tmp:
    write_video(tmp, args.frames)
    net, _ = build_net(Config, DEV)
    enc = MViT(arch="small", out_scales=[0, 1, 2, 3]).to(DEV).eval().requires_grad_(False)
    model = VideoSaliencyModel(channel_list=None, visual_net=enc, decoder_net=net).to(DEV).eval()
    sampler = DiffusionSampler(model, sample_type="ddim", timesteps=args.timesteps, noise_source="device")
    kw = dict(batch=args.batch, size=SIZE, len_snippet=args.len_snippet)
    clips = predict.list_clips("dhf1k", tmp, len_snippet=args.len_snippet)
    # warm-up: both loops over a short video of the same frame size (tables, packed weights, allocator pools, graph captures)
    warm = os.path.join(tmp, "warm")
    os.makedirs(os.path.join(warm, "frames"))
    os.makedirs(os.path.join(warm, "frames", "601"))
    n_warm = args.len_snippet + 2 * args.batch
    for i in range(1, n_warm + 1):
        os.link(os.path.join(tmp, "frames", "601", f"{i}.png"), os.path.join(warm, "frames", "601", f"{i}.png"))
    predict.predict_directory(model, sampler, "dhf1k", warm, os.path.join(tmp, "out_warm"), **kw)
    host_loop(sampler, predict.list_clips("dhf1k", warm, len_snippet=args.len_snippet), os.path.join(tmp, "out_warm_host"), args.batch)
    t_dev = timed(lambda: predict.predict_directory(model, sampler, "dhf1k", tmp, os.path.join(tmp, "out_dev"), videos=["601"], **kw))
    t_host = timed(lambda: host_loop(sampler, clips, os.path.join(tmp, "out_host"), args.batch))
    same = all(open(os.path.join(tmp, "out_dev", "601", f"{c.gt_index}.png"), "rb").read()
               == open(os.path.join(tmp, "out_host", "601", f"{c.gt_index}.png"), "rb").read() for c in clips)
    print(json.dumps({"frames": args.frames, "frame": [H, W], "size": list(SIZE), "clips": len(clips), "batch": args.batch,
                      "timesteps": args.timesteps, "len_snippet": args.len_snippet,
                      "predict_directory_s": t_dev, "predict_directory_clips_per_s": len(clips) / t_dev,
                      "host_loader_one_thread_s": t_host, "host_loader_one_thread_clips_per_s": len(clips) / t_host,
                      "files_identical": bool(same)}))
