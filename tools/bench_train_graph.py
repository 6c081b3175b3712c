#!/usr/bin/env python3
"""Eager against HIP-graph replay of the device-noise training step (DiffusionTrainStep(hip_graph=...)).

The full audio-visual model of BASELINE configs[3] (224 x 384, batch 4 per GPU) from synthetic weights and inputs, as bench.py's
train leg builds it, trained with ``noise_source="device"`` and the shipped loss configuration through ``loss_config``.  One
mode per call, timed in a fresh child process (no allocator, library or capture state from another mode):

    python tools/bench_train_graph.py --mode eager|graph [--steps 10] [--regions 5] [--warmup 4] [--batch 4] [--ids host|device]
                                      [--ema fused|helper] [--ema-rate 0.9999]

prints one JSON line: wall ms per step (median over the regions, each ``steps`` steps between two synchronisations), host ms per
step spent inside ``step()`` before the closing synchronise, the time of the call that captured, and
``torch.cuda.max_memory_allocated``.  ``--ids host`` (default) passes the sample ids as a Python list, as ``train``'s loop does;
the eager step uploads them from pageable memory, a copy that waits for the stream, so its host never runs more than a step
ahead.  ``--ids device`` passes an int64 GPU tensor.  ``--mode eager`` uses nothing newer than ``noise_source="device"``, so the
same file, copied beside an older checkout, times that checkout.  ``--ema fused`` trains with ``ema=<rate>`` (the shadow update
inside the clip + Adam kernel, either mode); ``--ema helper`` is the per-tensor form it replaces: a plain trainer and
``EMAHelper.update`` after every step, one ``axpbypcz`` launch per parameter tensor (eager only: its launches are not in a replay)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(mode, batch, dev, ema=None, ema_rate=0.9999):
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from diff_sal_amd.audio_attention import AudioAttnNet
    from diff_sal_amd.diff_model import VideoSaliencyModel
    from diff_sal_amd.mvit import MViT
    from diff_sal_amd.train_step import DiffusionTrainStep
    from diff_sal_amd.vggish import VGGish

    cfg = bench.Config()
    net, _ = bench.build_net(cfg, dev)
    H, W = cfg.img_size
    g = torch.Generator(device="cpu").manual_seed(4321)
    sal = torch.rand((batch, 1, H, W), generator=g).to(dev)
    torch.manual_seed(11)
    model = VideoSaliencyModel(channel_list=None, visual_net=MViT(arch="small", out_scales=[0, 1, 2, 3]), decoder_net=net,
                               audio_net=VGGish(pretrained=False),
                               spatiotemp_net=AudioAttnNet(depth=1, heads=2, dim=512, mlp_dim=256, patch_dim=512, num_patches=16,
                                                           height=7, width=12, pool="cls", dim_head=64)).to(dev)
    cond = {"img": torch.randn((batch, 3, 16, H, W), generator=g).to(dev),
            "audio": torch.randn((batch, 1, 9, H // 2, W // 2), generator=g).to(dev)}
    # the shipped loss configuration: the weighted MSE alone, through the loss dictionary
    loss = types.SimpleNamespace(loss_kl=False, kl_weight=1.0, loss_mse=True, mse_weight=1.0, loss_ce=False, ce_weight=1.0,
                                 loss_cc=False, cc_weight=-0.1, loss_sim=False, sim_weight=-0.1, loss_nss=False, nss_weight=-0.1)
    kw = dict(noise_source="device", seed=7, loss_config=types.SimpleNamespace(loss=loss))
    if mode == "graph":
        kw["hip_graph"] = True
    if ema == "fused":
        kw["ema"] = ema_rate
    return DiffusionTrainStep(model, **kw), sal, cond


def child(args):
    import torch

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ts, sal, cond = build(args.mode, args.batch, dev, args.ema, args.ema_rate)
    B, step, capture_ms = args.batch, 0, None
    helper = None
    if args.ema == "helper":
        from diff_sal_amd.ema import EMAHelper

        helper = EMAHelper(mu=args.ema_rate)
        helper.register(ts.model)
    id_base = torch.arange(B, dtype=torch.int64, device=dev)

    def one():
        nonlocal step
        ids = [step * B + i for i in range(B)] if args.ids == "host" else id_base + step * B
        step += 1
        loss = ts.step(sal, cond, sample_ids=ids)
        if helper is not None:
            helper.update(ts.model)
        return loss

    for _ in range(max(args.warmup, 3)):
        before = getattr(ts, "graph_captures", 0)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        one()
        torch.cuda.synchronize(dev)
        if getattr(ts, "graph_captures", 0) > before:
            capture_ms = (time.perf_counter() - t0) * 1e3
    wall, host = [], []
    for _ in range(args.regions):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            loss = one()
        t1 = time.perf_counter()
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        wall.append((t2 - t0) / args.steps * 1e3)
        host.append((t1 - t0) / args.steps * 1e3)
    out = {"tool": "bench_train_graph", "mode": args.mode, "ema": args.ema, "ema_rate": args.ema_rate if args.ema else None,
           "ema_tensors": None if helper is None else len(helper.shadow), "ids": args.ids, "batch": B, "steps": args.steps, "regions": args.regions,
           "wall_ms_per_step": round(statistics.median(wall), 3), "wall_ms_regions": [round(w, 3) for w in wall],
           "host_ms_per_step": round(statistics.median(host), 3), "capture_ms": None if capture_ms is None else round(capture_ms, 1),
           "max_memory_allocated_mb": round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1),
           "graph_captures": getattr(ts, "graph_captures", 0), "graph_replays": getattr(ts, "graph_replays", 0),
           "final_loss": float(loss.item()), "device": torch.cuda.get_device_name(dev)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("eager", "graph"), required=True)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--ids", choices=("host", "device"), default="host")
    ap.add_argument("--ema", choices=("fused", "helper"), default=None)
    ap.add_argument("--ema-rate", type=float, default=0.9999)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.ema == "helper" and args.mode == "graph":
        ap.error("--ema helper issues its launches from the host after the step: --mode eager only")
    if args.child:
        return child(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    return subprocess.call(cmd)


if __name__ == "__main__":
    sys.exit(main())
