"""proj_q and proj folded onto the key side of the 2 x Lk-key attention of the fp32 stages with C = 192 / 384 / 768
(ops.attn_fold, csrc/attn_fold.hip; SalUNet.fold_attn_proj): the operator against an fp64 evaluation in the reference's order,
that the fold is what runs in the network, network parity against the reference's fixtures with the switch on and off, and
determinism / per-frame independence."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import salunet_oracle as orc
from tests._cases import check_taps, load_case
from tests.test_gpu_salunet import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-3       # tests/test_gpu_salunet.py


def rnd(name, *shape, scale=1.0):
    return orc.synth_tensor(name, shape, scale)


def rel_err(got, ref):
    ref = ref.double().cpu()
    return (got.double().cpu() - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)


def _problem(C, L, Lk, n, tag=""):
    """Inputs of one block half: tokens, pooled rows, fan-in-scaled weights, biases of 0.1 sigma."""
    t = {k: rnd(f"af{tag}.{k}", n, l, C) for k, l in (("qin", L), ("kp", Lk), ("vp", Lk), ("x", L))}
    w = {k: rnd(f"af{tag}.W{k}", C, C, scale=C ** -0.5) for k in "qkvp"}
    b = {k: rnd(f"af{tag}.b{k}", C, scale=0.1) for k in "qkvp"}
    return t, w, b


def _folded_weights(w, b):
    from diff_sal_amd.sal_unet import SalUNet

    lin = lambda k: types.SimpleNamespace(weight=w[k].to(DEV), bias=b[k].to(DEV))
    return SalUNet.fold_attn_weights(types.SimpleNamespace(proj_q=lin("q"), proj_k=lin("k"), proj_v=lin("v"), proj=lin("p")))


def _run(ops, t, fw, C):
    kq, vp, ukq, bf = fw
    G, U = ops.linear_pair(t["kp"].to(DEV), t["vp"].to(DEV), kq, vp, None, None)
    return ops.attn_fold(t["qin"].to(DEV), G, U, t["kp"].to(DEV), ukq, t["x"].to(DEV), bf, 2, C ** -0.5), G, U


@pytest.mark.parametrize("C,L,Lk", [(768, 84, 18), (384, 336, 18), (192, 1344, 18), (192, 333, 18), (384, 8, 2), (768, 1, 2),
                                    (192, 200, 32)])
def test_attn_fold_against_fp64_reference_order(C, L, Lk):
    """q -> softmax -> o -> proj + residual in fp64 (the reference of tests/test_gpu_ops.py::test_attention_core, extended by the
    four projections).  Bar: the attention core's 2e-5; the CPU restatement of the fold in fp32 measures 2.5e-7, so the bar
    cannot hide a wrong mask or a dropped term.  Measured worst value over the seven shapes: 3.2e-7 (C = 384, L = 8, Lk = 2)."""
    from diff_sal_amd import ops

    n, heads = 3, 2
    t, w, b = _problem(C, L, Lk, n)
    d = C // heads
    td, wd, bd = ({k: v.double() for k, v in s.items()} for s in (t, w, b))
    q = td["qin"] @ wd["q"].T + bd["q"]
    k = td["kp"] @ wd["k"].T + bd["k"]
    v = td["vp"] @ wd["v"].T + bd["v"]
    qh, kh, vh = (z.reshape(n, -1, heads, d).transpose(1, 2) for z in (q, k, v))
    o = (F.softmax(qh @ kh.transpose(-1, -2) * C ** -0.5, -1) @ vh).transpose(1, 2).reshape(n, L, C)
    ref = o @ wd["p"].T + bd["p"] + td["x"]
    assert ops.attn_fold_supported(C, heads, Lk, torch.float32)
    got, _, _ = _run(ops, t, _folded_weights(w, b), C)
    err = rel_err(got, ref)
    print(f"attn_fold C={C} L={L} Lk={Lk}: rel err vs fp64 reference order {err:.3e}")
    assert err < 2e-5


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
    return sum(1 for _, note in recs if note.startswith("attn_fold"))


def test_the_fold_is_what_runs():
    """Reference configuration at the headline batch: three attn_fold launches and no K11 with the switch on; with it off no
    attn_fold, the three K11 launches of stages 0-2 and the five launches more that the fold removes (11 become 6)."""
    cfg = orc.SalUNetConfig()
    net = build(cfg, orc.synth_state_dict(orc.state_dict_template(cfg)))
    x, feats, _ = orc.synth_inputs(cfg, 4, False, tag="fold_ran")
    args = (x.to(DEV), torch.tensor([999, 650, 300, 0], device=DEV), [f.to(DEV) for f in feats], None)
    assert net.fold_attn_proj
    on = _ops_of(net, args)
    assert _n_fold(on) == 3 and not any(c == "K11" for c, _ in on)
    net.fold_attn_proj = False
    off = _ops_of(net, args)
    assert _n_fold(off) == 0 and sum(1 for c, _ in off if c == "K11") == 3
    assert len(off) == len(on) + 5


def _b4(golden_dir):
    cfg = orc.SalUNetConfig()
    g = np.load(f"{golden_dir}/salunet_full_vis_b4.npz")
    x, feats, _ = orc.synth_inputs(cfg, 4, False, tag="full_vis_b4")
    return cfg, orc.synth_state_dict(orc.state_dict_template(cfg)), x, torch.from_numpy(g["t"]), feats, None, g


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("name", ["full_vis_b4", "full_av_b1", "small_av", "small_vis"])
def test_network_parity_with_and_without_the_fold(golden_dir, name, fold):
    """Every stage* tap and the output against the reference's fixtures, inside the bar of tests/test_gpu_salunet.py, on both
    settings of the switch.  The small fixtures reach the kernel with 8 / 32 / 128 tokens and 2 keys per frame (tail masks,
    padded key rows)."""
    cfg, sd, x, t, feats, audio, g = _b4(golden_dir) if name == "full_vis_b4" else load_case(golden_dir, name)
    net = build(cfg, sd)
    net.fold_attn_proj = fold
    args = (x.to(DEV), t.to(DEV), [f.to(DEV) for f in feats], None if audio is None else audio.to(DEV))
    assert _n_fold(_ops_of(net, args)) == (3 if fold else 0)
    taps = {}
    with torch.no_grad():
        out = net(*args, taps=taps)
        out_fast = net(*args)
    ref = torch.from_numpy(g["output"])
    st = int(g["output_stride"]) if "output_stride" in g.files else 1
    errs = [(o.cpu()[:, :, ::st, ::st] - ref).abs().max().item() / ref.abs().max().item() for o in (out, out_fast)]
    worst = check_taps({k: net.tap_to_reference_layout(k, v) for k, v in taps.items() if k.startswith("stage")}, g, RTOL)
    print(f"{name} fold={int(fold)}: output rel err {errs[0]:.3e} / {errs[1]:.3e}; taps", {k: f"{v:.2e}" for k, v in worst.items()})
    assert {"stage0", "stage1", "stage2", "stage3"} <= set(worst)
    assert max(errs) < RTOL


@pytest.mark.parametrize("C,L,Lk", [(768, 84, 18), (192, 1344, 18), (384, 333, 7), (768, 1900, 18)])
def test_attn_fold_is_deterministic_and_frames_are_independent(C, L, Lk):
    """Two calls are bit-equal, and frame n of an N = 36 call is bit-equal to the same frame in an N = 1 call (the long
    shapes cross the library's choice of tokens per wave between the two calls)."""
    from diff_sal_amd import ops

    n = 36
    t, w, b = _problem(C, L, Lk, n, tag="det")
    fw = _folded_weights(w, b)
    got, G, U = _run(ops, t, fw, C)
    got2 = ops.attn_fold(t["qin"].to(DEV), G, U, t["kp"].to(DEV), fw[2], t["x"].to(DEV), fw[3], 2, C ** -0.5)
    assert torch.equal(got, got2)
    for f in (0, 17, 35):
        one = ops.attn_fold(t["qin"][f:f + 1].to(DEV), G[f:f + 1].contiguous(), U[f:f + 1].contiguous(), t["kp"][f:f + 1].to(DEV),
                            fw[2], t["x"][f:f + 1].to(DEV), fw[3], 2, C ** -0.5)
        assert torch.equal(one[0], got[f])
