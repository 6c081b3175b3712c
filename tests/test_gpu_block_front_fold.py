"""proj_q and proj folded onto the key side inside the fused block front of the fp32 C = 96 stage (ops.block_front_fold,
csrc/tblock.hip; SalUNet.fold_front_proj): the operator against an fp64 evaluation in the reference's order and against
ops.block_front, determinism / per-frame independence / equality of the two occupancy variants, that the fold is what runs in the
network, network parity against the reference's fixtures on both settings of the switch, and (no GPU) the algebra of the folded
weights at C = 96."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import salunet_oracle as orc

DEV = "cuda"
RTOL = 1e-3       # tests/test_gpu_salunet.py
C96_SHAPES = [(3, 16, 32, 18), (2, 8, 16, 2), (2, 13, 21, 18), (36, 56, 96, 18), (1, 5, 7, 32)]   # tests/test_gpu_block_front.py


def rnd(name, *shape, scale=1.0):
    return orc.synth_tensor(name, shape, scale)


def _problem(N, H, W, Lk, C=96, tag="ff"):
    """Inputs scaled as in tests/test_gpu_block_front.py; weights with fan-in scale and biases of 0.1 sigma as in
    tests/test_gpu_attn_fold.py."""
    t = f"{tag}{H}."
    p = dict(g1=rnd(t + "g1", C, scale=0.1) + 1, b1=rnd(t + "b1", C, scale=0.1), w9=rnd(t + "w9", 9, C, scale=0.4),
             gq=rnd(t + "gq", C, scale=0.1) + 1, bq=rnd(t + "bq", C, scale=0.1))
    x = rnd(t + "x", N, H, W, C) * 1.5 + 0.2
    kp, vp = rnd(t + "kp", N, Lk, C, scale=1.2), rnd(t + "vp", N, Lk, C)
    w = {k: rnd(t + "W" + k, C, C, scale=C ** -0.5) for k in "qkvp"}
    b = {k: rnd(t + "B" + k, C, scale=0.1) for k in "qkvp"}
    return x, kp, vp, p, w, b


def _lin_ns(w, b, dev):
    lin = lambda k: types.SimpleNamespace(weight=w[k].to(dev), bias=b[k].to(dev))
    return types.SimpleNamespace(proj_q=lin("q"), proj_k=lin("k"), proj_v=lin("v"), proj=lin("p"))


def _reference64(x, kp, vp, p, w, b, heads=2):
    """LayerNorm -> depthwise 3x3 -> LayerNorm -> proj_q, proj_k / proj_v of the pooled rows -> per-head softmax with scale C^-1/2
    -> proj + residual, all in fp64."""
    x, kp, vp = x.double(), kp.double(), vp.double()
    p, w, b = ({k: v.double() for k, v in s.items()} for s in (p, w, b))
    N, H, W, C = x.shape
    xn = F.layer_norm(x, (C,), p["g1"], p["b1"], 1e-5)
    qd = F.conv2d(xn.permute(0, 3, 1, 2), p["w9"].t().reshape(C, 1, 3, 3), None, padding=1, groups=C).permute(0, 2, 3, 1)
    qin = F.layer_norm(qd, (C,), p["gq"], p["bq"], 1e-5).reshape(N, H * W, C)
    q, k, v = qin @ w["q"].T + b["q"], kp @ w["k"].T + b["k"], vp @ w["v"].T + b["v"]
    d = C // heads
    qh, kh, vh = (z.reshape(N, -1, heads, d).transpose(1, 2) for z in (q, k, v))
    o = (F.softmax(qh @ kh.transpose(-1, -2) * float(C) ** -0.5, -1) @ vh).transpose(1, 2).reshape(N, H * W, C)
    return (o @ w["p"].T + b["p"]).reshape(N, H, W, C) + x


def _run_fold(ops, x, kp, vp, p, fw, wgs=None):
    """wgs = 1: the one-workgroup form (tuning switch DIFFSAL_FRONT_FOLD_WGS), else the shipped two-workgroup form."""
    from diff_sal_amd import _lib

    kq, vpw, ukq, bf = fw
    d = lambda t: t.to(DEV)
    G, U = ops.linear_pair(d(kp), d(vp), kq, vpw, None, None)
    C = x.shape[-1]
    _lib.set_tuning("DIFFSAL_FRONT_FOLD_WGS", wgs)
    try:
        return ops.block_front_fold(d(x), G, U, d(kp), ukq, (d(p["g1"]), d(p["b1"]), 1e-5), d(p["w9"]), (d(p["gq"]), d(p["bq"]), 1e-5),
                                    bf, 2, float(C) ** -0.5)
    finally:
        _lib.set_tuning("DIFFSAL_FRONT_FOLD_WGS", None)


def _rel(got, ref):
    ref = ref.double().cpu()
    return (got.double().cpu() - ref).abs().max().item() / ref.abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", C96_SHAPES)
def test_block_front_fold_against_fp64_reference_order(shape):
    """Bar 2e-5 of the output maximum (the fp32 bar of tests/test_gpu_block_front.py for this chain).  A CPU restatement of the fold
    in fp32 measures 0.9e-7 to 1.5e-7 on these shapes and the reference's own order in fp32 0.8e-7 to 1.5e-7, so the bar cannot hide
    a wrong mask or a dropped term."""
    from diff_sal_amd import ops
    from diff_sal_amd.sal_unet import SalUNet

    N, H, W, Lk = shape
    x, kp, vp, p, w, b = _problem(N, H, W, Lk)
    assert ops.block_front_fold_supported(96, 2, Lk, torch.float32)
    ref = _reference64(x, kp, vp, p, w, b)
    fw = SalUNet.fold_attn_weights(_lin_ns(w, b, DEV))
    for variant in (None, 1):
        got = _run_fold(ops, x, kp, vp, p, fw, variant)
        torch.cuda.synchronize()
        assert got.shape == ref.shape and got.dtype == torch.float32
        err = _rel(got, ref)
        print(f"block_front_fold {shape} workgroups per CU {variant or 2}: rel err vs fp64 reference order {err:.3e}")
        assert err < 2e-5


@pytest.mark.gpu
@pytest.mark.parametrize("shape", C96_SHAPES)
def test_block_front_fold_equals_block_front(shape):
    """Both operators on the same inputs; block_front gets k and v from linear_pair with the unfolded weights.  Bar: the 1e-5 of
    test_block_front_equals_unfused_hip_kernels."""
    from diff_sal_amd import ops
    from diff_sal_amd.sal_unet import SalUNet

    N, H, W, Lk = shape
    x, kp, vp, p, w, b = _problem(N, H, W, Lk, tag="fe")
    d = lambda t: t.to(DEV)
    k, v = ops.linear_pair(d(kp), d(vp), d(w["k"]), d(w["v"]), d(b["k"]), d(b["v"]))
    want = ops.block_front(d(x), k, v, (d(p["g1"]), d(p["b1"]), 1e-5), d(p["w9"]), (d(p["gq"]), d(p["bq"]), 1e-5),
                           (d(w["q"]), d(b["q"])), (d(w["p"]), d(b["p"])), 2, 96.0 ** -0.5)
    got = _run_fold(ops, x, kp, vp, p, SalUNet.fold_attn_weights(_lin_ns(w, b, DEV)))
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"block_front_fold vs block_front {shape}: rel err {err:.3e}")
    assert err < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,Lk", [(56, 96, 18), (13, 21, 18), (16, 32, 7)])
def test_block_front_fold_is_deterministic_and_frames_are_independent(H, W, Lk):
    """Two calls are bit-equal; frame n of an N = 36 call is bit-equal to the same frame in an N = 1 call; the one- and the
    two-workgroup variants are bit-equal."""
    from diff_sal_amd import ops
    from diff_sal_amd.sal_unet import SalUNet

    N = 36
    x, kp, vp, p, w, b = _problem(N, H, W, Lk, tag="fd")
    fw = SalUNet.fold_attn_weights(_lin_ns(w, b, DEV))
    got = _run_fold(ops, x, kp, vp, p, fw)
    assert torch.equal(got, _run_fold(ops, x, kp, vp, p, fw))
    assert torch.equal(got, _run_fold(ops, x, kp, vp, p, fw, 1))
    for f in (0, 17, 35):
        for variant in (None, 1):
            one = _run_fold(ops, x[f:f + 1], kp[f:f + 1], vp[f:f + 1], p, fw, variant)
            assert torch.equal(one[0], got[f])


def _ops_of(net, args):
    from diff_sal_amd import ops

    ops.PROFILE = []
    try:
        with torch.no_grad():
            net(*args)
        torch.cuda.synchronize()
        return [(p[3], p[5]) for p in ops.PROFILE]
    finally:
        ops.PROFILE = None


def _n_fold(recs):
    return sum(1 for _, note in recs if note.startswith("block_front_fold M="))


def _n_plain(recs):
    return sum(1 for _, note in recs if note.startswith("block_front M="))


@pytest.mark.gpu
def test_the_fold_is_what_runs():
    """Reference configuration at the headline batch: exactly one block_front_fold record and no block_front record with the switch
    on, the reverse with it off, and the same number of launches on both settings."""
    from tests.test_gpu_salunet import build

    cfg = orc.SalUNetConfig()
    net = build(cfg, orc.synth_state_dict(orc.state_dict_template(cfg)))
    x, feats, _ = orc.synth_inputs(cfg, 4, False, tag="front_fold_ran")
    args = (x.to(DEV), torch.tensor([999, 650, 300, 0], device=DEV), [f.to(DEV) for f in feats], None)
    assert net.fold_front_proj
    on = _ops_of(net, args)
    assert _n_fold(on) == 1 and _n_plain(on) == 0
    net.fold_front_proj = False
    off = _ops_of(net, args)
    assert _n_fold(off) == 0 and _n_plain(off) == 1
    assert len(on) == len(off)


def _b4(golden_dir):
    cfg = orc.SalUNetConfig()
    g = np.load(f"{golden_dir}/salunet_full_vis_b4.npz")
    x, feats, _ = orc.synth_inputs(cfg, 4, False, tag="full_vis_b4")
    return cfg, orc.synth_state_dict(orc.state_dict_template(cfg)), x, torch.from_numpy(g["t"]), feats, None, g


@pytest.mark.gpu
@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("name", ["full_vis_b4", "full_av_b1", "small_av", "small_vis"])
def test_network_parity_with_and_without_the_front_fold(golden_dir, name, fold):
    """Every stage* tap and the output against the reference's fixtures, inside the bar of tests/test_gpu_salunet.py, on both
    settings of the switch.  The AV fixtures take the keys from the audio-fused frames."""
    from tests._cases import check_taps, load_case
    from tests.test_gpu_salunet import build

    cfg, sd, x, t, feats, audio, g = _b4(golden_dir) if name == "full_vis_b4" else load_case(golden_dir, name)
    net = build(cfg, sd)
    net.fold_front_proj = fold
    args = (x.to(DEV), t.to(DEV), [f.to(DEV) for f in feats], None if audio is None else audio.to(DEV))
    recs = _ops_of(net, args)
    assert _n_fold(recs) + _n_plain(recs) == 1 and _n_fold(recs) == int(fold)
    taps = {}
    with torch.no_grad():
        out = net(*args, taps=taps)
        out_fast = net(*args)
    ref = torch.from_numpy(g["output"])
    st = int(g["output_stride"]) if "output_stride" in g.files else 1
    errs = [(o.cpu()[:, :, ::st, ::st] - ref).abs().max().item() / ref.abs().max().item() for o in (out, out_fast)]
    worst = check_taps({k: net.tap_to_reference_layout(k, v) for k, v in taps.items() if k.startswith("stage")}, g, RTOL)
    print(f"{name} front fold={int(fold)}: output rel err {errs[0]:.3e} / {errs[1]:.3e}; taps", {k: f"{v:.2e}" for k, v in worst.items()})
    assert {"stage0", "stage1", "stage2", "stage3"} <= set(worst)
    assert max(errs) < RTOL


def test_folded_weights_reproduce_the_block_half_in_fp64_at_c96():
    """No GPU: with SalUNet.fold_attn_weights(dtype=float64) the key-side form equals q -> softmax -> o -> proj + residual in fp64.
    Bar 1e-13 of the output maximum: fp64 rounding (1.1e-16) through two chained contractions of length 96 and a softmax of
    scores of order one stays two orders below it, and a dropped or misplaced term is of order one.  The fp32 result the network
    packs is that fp64 result rounded once."""
    from diff_sal_amd.sal_unet import SalUNet

    C, heads, n, L, Lk = 96, 2, 3, 77, 18
    d = C // heads
    g = torch.Generator().manual_seed(96)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g, dtype=torch.float64) * sc
    qin, kp, vp, x = r(n, L, C), r(n, Lk, C, sc=1.2), r(n, Lk, C), r(n, L, C)
    w = {k: r(C, C, sc=C ** -0.5).float() for k in "qkvp"}      # fp32 parameters, as the module holds them
    b = {k: r(C, sc=0.1).float() for k in "qkvp"}
    wd, bd = ({k: v.double() for k, v in s.items()} for s in (w, b))
    q, k, v = qin @ wd["q"].T + bd["q"], kp @ wd["k"].T + bd["k"], vp @ wd["v"].T + bd["v"]
    qh, kh, vh = (z.reshape(n, -1, heads, d).transpose(1, 2) for z in (q, k, v))
    o = (torch.softmax(qh @ kh.transpose(-1, -2) * C ** -0.5, -1) @ vh).transpose(1, 2).reshape(n, L, C)
    ref = o @ wd["p"].T + bd["p"] + x
    kq, vpw, ukq, bf = SalUNet.fold_attn_weights(_lin_ns(w, b, "cpu"), dtype=torch.float64)
    assert kq.shape == (2 * C, C) and vpw.shape == (2 * C, C) and ukq.shape == (heads, C) and bf.shape == (C,)
    G, U = (kp @ kq.T).reshape(n, Lk, heads, C), (vp @ vpw.T).reshape(n, Lk, heads, C)
    acc = x + bf
    for h in range(heads):
        s = (qin @ G[:, :, h].transpose(-1, -2) + (kp @ ukq[h])[:, None, :]) * C ** -0.5
        acc = acc + torch.softmax(s, -1) @ U[:, :, h]
    err = (acc - ref).abs().max().item() / ref.abs().max().item()
    print(f"folded weights at C = 96 in fp64: rel err {err:.3e}")
    assert err < 1e-13
    for a32, a64 in zip(SalUNet.fold_attn_weights(_lin_ns(w, b, "cpu")), (kq, vpw, ukq, bf)):
        assert a32.dtype == torch.float32 and torch.equal(a32, a64.float())


def test_folded_front_kernels_use_no_scratch():
    """No GPU: the two-workgroup form fits its 256 registers only because the per-thread piece offsets are kept out of the tile
    loop's invariants (csrc/tblock.hip); a toolchain that hoists them again would spill silently.  The code object's metadata
    (tools/check_scratch.py) must list neither instantiation with a private segment."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf of the ROCm toolchain not found")
    from diff_sal_amd import _lib

    _lib.load()      # builds the library if it is missing
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "check_scratch.py")], capture_output=True, text=True, check=True).stdout
    assert "kernels with scratch" in out
    assert not [l for l in out.splitlines() if "block_front_fold_kernel" in l], out
