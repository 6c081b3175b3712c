#!/usr/bin/env python3
"""Time diffsal_block_front (csrc/tblock.hip) at the finest decoder stage's shape, beside the unfused launches it replaces.  GPU only."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sal_amd import _lib, ops  # noqa: E402


def timed(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def fold_leg(x, kp, vp, norm1, w9, norm_q, r, unfolded):
    """ops.block_front_fold (proj_q / proj on the key side) beside ops.block_front on the same tokens: the shipped form, the one-
    and the two-workgroup variants, and the paired product that feeds each (N = C against N = 2 C); interleaved rounds, median."""
    N, H, W, C = x.shape
    wk, wv = r(C, C, sc=C ** -0.5), r(C, C, sc=C ** -0.5)
    kq, vpw, ukq, bf = r(2 * C, C, sc=C ** -0.5), r(2 * C, C, sc=C ** -0.5), r(2, C, sc=0.1), r(C, sc=0.1)
    bk, bv = r(C, sc=0.1), r(C, sc=0.1)
    G, U = ops.linear_pair(kp, vp, kq, vpw, None, None)
    fold = lambda: ops.block_front_fold(x, G, U, kp, ukq, norm1, w9, norm_q, bf, 2, C ** -0.5)

    def fold_one_wg():      # timed() synchronises before it returns: the switch covers exactly its launches
        _lib.set_tuning("DIFFSAL_FRONT_FOLD_WGS", 1)
        try:
            return timed(fold)
        finally:
            _lib.set_tuning("DIFFSAL_FRONT_FOLD_WGS", None)

    legs = {"block_front": unfolded, "fold, 2 workgroups / CU (shipped)": fold, "fold, 1 workgroup / CU": None,
            "linear_pair N = C": lambda: ops.linear_pair(kp, vp, wk, wv, bk, bv),
            "linear_pair N = 2C": lambda: ops.linear_pair(kp, vp, kq, vpw, None, None)}
    times = {k_: [] for k_ in legs}
    for _ in range(7):
        for k_, fn in legs.items():
            times[k_].append(timed(fn) if fn is not None else fold_one_wg())
    for k_, t in times.items():
        t.sort()
        print(f"{'':15s} {k_:34s} median {t[len(t) // 2]:7.1f} us   min {t[0]:7.1f}   max {t[-1]:7.1f}")


def main():
    Lk, heads = 18, 2
    scale = int(os.environ.get("FRONT_SCALE", "1"))       # 16: the 64-clip pass
    for dt, (N, H, W, C) in ((torch.float32, (36, 56, 96, 96)), (torch.bfloat16, (36, 56, 96, 96)), (torch.float16, (36, 56, 96, 96)),
                             (torch.bfloat16, (36, 28, 48, 192)), (torch.float16, (36, 28, 48, 192))):
        N *= scale
        g = torch.Generator(device="cuda").manual_seed(0)
        r = lambda *s, sc=1.0: torch.randn(*s, device="cuda", generator=g) * sc
        x = r(N, H, W, C).to(dt)
        k, v = r(N, Lk, C).to(dt), r(N, Lk, C).to(dt)
        g1, b1, gq, bq = r(C, sc=0.1) + 1, r(C, sc=0.1), r(C, sc=0.1) + 1, r(C, sc=0.1)
        w9 = r(9, C, sc=0.4)
        wq, wp = r(C, C, sc=C ** -0.5).to(dt), r(C, C, sc=C ** -0.5).to(dt)
        biq, bip = r(C, sc=0.1), r(C, sc=0.1)
        f32 = dt == torch.float32
        fused = lambda: ops.block_front(x, k, v, (g1, b1, 1e-5), w9, (gq, bq, 1e-5), (wq, biq), (wp, bip) if f32 else None, heads, C ** -0.5)

        def unfused():
            xn = ops.layernorm(x, g1, b1, 1e-5)
            q = ops.dwconv3_ln(xn, w9, gq, bq, 1e-5)
            q = ops.linear(q, wq, biq)
            o = ops.attention(q, k, v, heads, C ** -0.5)
            if f32:
                return ops.linear(o, wp, bip, residual=x.view(N, H * W, C))
            return o

        M = N * H * W
        tf, tu = timed(fused), timed(unfused)
        nb = 2 * M * C * x.element_size()
        print(f"{str(dt):15s} C={C} M={M}: fused {tf:7.1f} us ({nb / tf / 1e3:6.0f} GB/s once-through)   unfused {tu:7.1f} us")
        if f32 and ops.block_front_fold_supported(C, heads, Lk, dt):
            fold_leg(x, k, v, (g1, b1, 1e-5), w9, (gq, bq, 1e-5), r, fused)
        if C != 96:
            continue
        # the block's second half on the same tokens
        w1, b1_, w2, b2_ = r(2 * C, C, sc=0.1).to(dt), r(2 * C, sc=0.1), r(C, 2 * C, sc=0.08).to(dt), r(C, sc=0.1)
        xt = x.view(N, H * W, C)
        geom = (H * W, 9, 5)
        if f32:
            tb = timed(lambda: ops.mlp_block(xt, (g1, b1, 1e-5), (w1, b1_), (w2, b2_), (gq, bq, 1e-5), geom))
            print(f"{'':15s} mlp_block (LN + fc1 + GELU + fc2 + res + norm_mts): {tb:7.1f} us  {8 * M * C * C / tb / 1e6:6.1f} TF/s")
        else:
            tb = timed(lambda: ops.block16(xt, xt, (wp, bip), (g1, b1, 1e-5), (w1, b1_), (w2, b2_), (gq, bq, 1e-5), geom))
            print(f"{'':15s} block16 (proj + res + LN + MLP + res + norm_mts): {tb:7.1f} us  {10 * M * C * C / tb / 1e6:6.1f} TF/s")


if __name__ == "__main__":
    main()
