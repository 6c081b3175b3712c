"""Norms, softmax and activations beyond unit-normal inputs (cases, references and tolerances: tests/_value_range_ref.py).

A. normalisation under a mean offset R (x = z + R o, o = +-1 alternating by group / row / channel), every form of GroupNorm;
B. softmax with logits scaled by 1, 16 and 128, all keys equal, and a one-hot row;
C. every activation over [-40, 40] plus the edges of the float range, fed through identity weights so that the activation sees
   exactly the swept values; +-inf and NaN through the element-wise entries;
D. constant and all-zero rows through the normalisations of A.

Every case prints its error, its bound and the ratio of its error to the fp32 torch reference's own error."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _value_range_ref as vr

pytestmark = pytest.mark.gpu
DEV = "cuda"


def to_dev(t):
    """The upload of the shared case bodies; tests/test_gpu_guard_bands.py passes tests/_guard.py's ``put`` in its place."""
    return t.to(DEV)


def dv(t, dname="fp32", up=to_dev):
    return up(t.detach().to(DEV).to(vr.DTYPES[dname]))


def ids(cases):
    return [c.id for c in cases]


@pytest.fixture(scope="module")
def ops():
    from diff_sal_amd import ops as o

    assert torch.cuda.is_available()
    return o


@pytest.fixture(scope="module")
def agops():
    from diff_sal_amd import autograd_ops

    return autograd_ops


def last_kernel():
    from diff_sal_amd import _lib

    return _lib.load().diffsal_last_gemm_kernel().decode()


# ------------------------------------------------------------------------------------------------------------------------
# A / D: GroupNorm
# ------------------------------------------------------------------------------------------------------------------------
GN_FORMS = {"default": {}, "two-launch": {"DIFFSAL_NO_GN_SLAB": 1}, "two-launch-1-chunk": {"DIFFSAL_NO_GN_SLAB": 1, "DIFFSAL_GN_CHUNKS": 1},
            "two-launch-128-chunks": {"DIFFSAL_NO_GN_SLAB": 1, "DIFFSAL_GN_CHUNKS": 128}}
GN_SWISH = [c for c in vr.gn_cases() + vr.gn_gain_cases() if c.id.startswith("gn_swish")]
GN_LEGACY = [c for c in vr.gn_cases() if c.id.startswith("gn_legacy")]


def gn_forms_of(case):
    return list(GN_FORMS) if case.p["dname"] == "fp32" and case.p["gain"] == 1.0 else ["default", "two-launch"]


@pytest.mark.parametrize("case,form", [(c, f) for c in GN_SWISH for f in gn_forms_of(c)],
                         ids=["%s-%s" % (c.id, f) for c in GN_SWISH for f in gn_forms_of(c)])
def test_groupnorm_swish_every_form(ops, tuning, case, form):
    """The slab kernel where the shape admits it (B * groups >= 128: only the 4-image shape, in all three storage types; below that
    "default" is the two-launch path as well; two-pass) and the statistics + normalisation launches (sums about a pivot) satisfy one bound; 1 chunk of (1,56,96,96) gives a thread hundreds of terms.  gain32: gamma = 32, so
    that swish sees about +-120 (part C)."""
    for k, v in GN_FORMS[form].items():
        tuning.set(k, v)
    t, _, _ = vr.evaluate(case)
    dn = case.p["dname"]
    got = ops.groupnorm_swish(dv(t["x"], dn), dv(t["g"]), dv(t["b"]), 32, vr.GN_EPS)
    assert got.dtype == vr.DTYPES[dn]
    ran = form if form != "default" else ("slab" if case.p["shape"][0] * 32 >= 128 else "two-launch, as the library chooses")
    vr.check(case, dict(y=got), "groupnorm_swish[%s,%s]" % (ran, dn))


@pytest.mark.parametrize("case", GN_LEGACY, ids=ids(GN_LEGACY))
def test_groupnorm_legacy_entry(ops, case):
    t, _, _ = vr.evaluate(case)
    got = ops.groupnorm(dv(t["x"]), dv(t["g"]), dv(t["b"]), 32, vr.GN_EPS, swish=case.p["swish"])
    vr.check(case, dict(y=got), "groupnorm[swish=%d]" % case.p["swish"])


GN_PLAIN = [c for c in GN_LEGACY if not c.p["swish"]]


@pytest.mark.parametrize("case", GN_PLAIN, ids=[c.id.replace("gn_legacy-swish0", "gn_affine") for c in GN_PLAIN])
def test_gn_affine_rows(ops, case):
    """x a + b formed in fp64 from the returned fp32 rows against the fp64 GroupNorm"""
    t, _, _ = vr.evaluate(case)
    ab = ops.gn_affine(dv(t["x"]), dv(t["g"]), dv(t["b"]), 32, vr.GN_EPS).double().cpu()
    y = t["x"].double() * ab[:, 0][:, None, None, :] + ab[:, 1][:, None, None, :]
    vr.check(case, dict(y=y), "gn_affine")


GN_TRAIN = vr.gn_train_cases()


def case_groupnorm_swish_training(agops, case, up=to_dev):
    t, _, _ = vr.evaluate(case)
    x, g, b = (dv(t[k], up=up).requires_grad_(True) for k in ("x", "g", "b"))
    y = agops.groupnorm_swish(x, g, b, 32, vr.GN_EPS)
    y.backward(dv(t["dy"], up=up))
    vr.check(case, dict(y=y, dx=x.grad, dgamma=g.grad, dbeta=b.grad), "autograd groupnorm_swish")


@pytest.mark.parametrize("case", GN_TRAIN, ids=ids(GN_TRAIN))
def test_groupnorm_swish_training(agops, case):
    case_groupnorm_swish_training(agops, case)


BN = vr.bn_cases()


def case_batchnorm_training(agops, case, up=to_dev):
    t, _, _ = vr.evaluate(case)
    bn = torch.nn.BatchNorm2d(vr.BN_C, eps=vr.BN_EPS, momentum=0.1).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(t["g"])
        bn.bias.copy_(t["b"])
        bn.running_mean.copy_(t["rm"])
        bn.running_var.copy_(t["rv"])
    for t_ in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
        t_.data = up(t_.data)
    x = dv(t["x"], up=up).requires_grad_(True)
    y = agops.batchnorm_relu_train(x, bn, relu=case.p["relu"])
    y.backward(dv(t["dy"], up=up))
    vr.check(case, dict(y=y, running_mean=bn.running_mean, running_var=bn.running_var, dx=x.grad, dgamma=bn.weight.grad,
                        dbeta=bn.bias.grad), "autograd batchnorm_relu_train")


@pytest.mark.parametrize("case", BN, ids=ids(BN))
def test_batchnorm_training(agops, case):
    case_batchnorm_training(agops, case)


# ------------------------------------------------------------------------------------------------------------------------
# A / D: LayerNorm (every one two-pass: these pin that)
# ------------------------------------------------------------------------------------------------------------------------
LN = vr.ln_cases()


@pytest.mark.parametrize("case", LN, ids=ids(LN))
def test_layernorm(ops, case):
    t, _, _ = vr.evaluate(case)
    dn = case.p["dname"]
    got = ops.layernorm(dv(t["x"], dn), dv(t["g"]), dv(t["b"]), vr.LN_EPS)
    assert got.dtype == vr.DTYPES[dn]
    vr.check(case, dict(y=got), "layernorm[%s]" % dn)


LN_MULTI = vr.ln_multi_cases()


@pytest.mark.parametrize("case", LN_MULTI, ids=ids(LN_MULTI))
def test_layernorm_multi(ops, case):
    t, _, _ = vr.evaluate(case)
    n = len(vr.LN_MULTI_ROWS)
    outs = ops.layernorm_multi([dv(t["x%d" % i]) for i in range(n)], [dv(t["g%d" % i]) for i in range(n)],
                               [dv(t["b%d" % i]) for i in range(n)], [vr.LN_EPS] * n)
    vr.check(case, {"y%d" % i: o for i, o in enumerate(outs)}, "layernorm_multi")


LN_BWD = vr.ln_bwd_cases()


@pytest.mark.parametrize("case", LN_BWD, ids=ids(LN_BWD))
def test_layernorm_backward(agops, case):
    t, _, _ = vr.evaluate(case)
    x, g, b = (dv(t[k]).requires_grad_(True) for k in ("x", "g", "b"))
    if case.p["fork"]:
        xr, y = agops.layernorm_fork(x, g, b, vr.LN_EPS)
        (y + 1.5 * xr).backward(dv(t["dy"]))
    else:
        agops.layernorm(x, g, b, vr.LN_EPS).backward(dv(t["dy"]))
    vr.check(case, dict(dx=x.grad, dgamma=g.grad, dbeta=b.grad), "autograd layernorm_fork" if case.p["fork"] else "autograd layernorm")


# ------------------------------------------------------------------------------------------------------------------------
# B: softmax
# ------------------------------------------------------------------------------------------------------------------------
ATTN = vr.attn_cases()
ATTN_RUNS = [(c, m) for c in ATTN for m in ((None,) if c.p["dname"] == "fp32" else (None, 1))]


@pytest.mark.parametrize("case,no_mfma", ATTN_RUNS, ids=["%s%s" % (c.id, "-no-mfma" if m else "") for c, m in ATTN_RUNS])
def test_attention(ops, tuning, case, no_mfma):
    """a = 128 puts the logits past +-300: exp overflows unless the row maximum is subtracted first"""
    if no_mfma:
        tuning.set("DIFFSAL_NO_ATTN16_MFMA", 1)
    t, _, _ = vr.evaluate(case)
    p = case.p
    got = ops.attention(dv(t["q"], p["dname"]), dv(t["k"], p["dname"]), dv(t["v"], p["dname"]), p["heads"], p["C"] ** -0.5)
    vr.check(case, dict(o=got), "attention[%s%s]" % (p["dname"], ",no-mfma" if no_mfma else ""))


ATTN_BWD = vr.attn_bwd_cases()


@pytest.mark.parametrize("case", ATTN_BWD, ids=ids(ATTN_BWD))
def test_attention_backward(ops, agops, case):
    t, _, _ = vr.evaluate(case)
    p = case.p
    scale = p["C"] ** -0.5
    dq, dk, dv_ = ops.attention_bwd(dv(t["q"]), dv(t["k"]), dv(t["v"]), dv(t["do"]), p["heads"], scale)
    vr.check(case, dict(dq=dq, dk=dk, dv=dv_), "attention_bwd")
    qq, kk, vv = (dv(t[k]).requires_grad_(True) for k in "qkv")
    agops.attention(qq, kk, vv, p["heads"], scale).backward(dv(t["do"]))
    vr.check(case, dict(dq=qq.grad, dk=kk.grad, dv=vv.grad), "autograd attention")


ATTN_GENERAL = vr.attn_general_cases()


@pytest.mark.parametrize("case", ATTN_GENERAL, ids=ids(ATTN_GENERAL))
def test_attention_general_forward_lse_and_both_backward_forms(ops, case):
    t, _, _ = vr.evaluate(case)
    E = case.p["shape"][5]
    qq, kk, vv = dv(t["q"]), dv(t["k"]), dv(t["v"])
    kw = dict(scale=case.p["shape"][4] ** -0.5, q_extra=dv(t["qe"]) if E else None, k_extra=dv(t["ke"]) if E else None,
              residual=qq if E else None, skip_first=bool(E))
    out, lse = ops.attention_general(qq, kk, vv, want_lse=True, **kw)
    vr.check(case, dict(o=out, lse=lse), "attention_general")
    for ds_form in (False, True):
        dq, dqe, dk, dv_ = ops.attention_general_bwd(qq, kk, vv, out, lse, dv(t["do"]), ds_form=ds_form, **kw)
        got = dict(dq=dq, dk=dk, dv=dv_)
        if E:
            got["dqe"] = dqe
        vr.check(case, got, "attention_general_bwd[ds_form=%d]" % ds_form)


SOFTMAX = vr.softmax_cases()


@pytest.mark.parametrize("case", SOFTMAX, ids=ids(SOFTMAX))
def test_softmax_rows(ops, case):
    t, _, _ = vr.evaluate(case)
    vr.check(case, dict(y=ops.softmax_rows(dv(t["x"]), 0.7)), "softmax_rows")


ATTN_FOLD = vr.attn_fold_cases()


@pytest.mark.parametrize("case", ATTN_FOLD, ids=ids(ATTN_FOLD))
def test_attn_fold(ops, case):
    from tests.test_gpu_attn_fold import _folded_weights, _run

    inp, _, _ = vr.evaluate(case)
    got, _, _ = _run(ops, inp["t"], _folded_weights(inp["w"], inp["b"]), case.p["C"])
    vr.check(case, dict(y=got), "attn_fold")


FRONT = vr.front_cases()


@pytest.mark.parametrize("case", FRONT, ids=ids(FRONT))
def test_block_front_and_its_fold(ops, case):
    """A: the two LayerNorms inside the fused block front under offset token rows; B: its softmax with the pooled key rows scaled.
    block_front gets k and v from linear_pair with the unfolded weights, block_front_fold the folded ones (both variants)."""
    from diff_sal_amd.sal_unet import SalUNet
    from tests.test_gpu_block_front_fold import _lin_ns, _run_fold

    t, _, _ = vr.evaluate(case)
    x, kp, vp, p, w, b = (t[k] for k in ("x", "kp", "vp", "prm", "w", "b"))
    k, v = ops.linear_pair(dv(kp), dv(vp), dv(w["k"]), dv(w["v"]), dv(b["k"]), dv(b["v"]))
    got = ops.block_front(dv(x), k, v, (dv(p["g1"]), dv(p["b1"]), 1e-5), dv(p["w9"]), (dv(p["gq"]), dv(p["bq"]), 1e-5),
                          (dv(w["q"]), dv(b["q"])), (dv(w["p"]), dv(b["p"])), 2, 96.0 ** -0.5)
    vr.check(case, dict(y=got), "block_front")
    fw = SalUNet.fold_attn_weights(_lin_ns(w, b, DEV))
    for variant in (None, 1):
        vr.check(case, dict(y=_run_fold(ops, x, kp, vp, p, fw, variant)), "block_front_fold")


MLP = vr.mlp_cases()


@pytest.mark.parametrize("case", MLP, ids=ids(MLP))
def test_mlp_block_and_block16(ops, case):
    """A: norm2 and norm_mts inside the fused MLP kernels under offset token rows; C (gain32): GELU sees about +-100"""
    t, _, _ = vr.evaluate(case)
    p = case.p
    dn = p["dname"]
    args = ((dv(t["g2"]), dv(t["b2n"]), 1e-5), (dv(t["w1"], dn), dv(t["bb1"])), (dv(t["w2"], dn), dv(t["bb2"])),
            (dv(t["gz"]), dv(t["bz"]), 1e-5), vr.MLP_FRAMES)
    if p["op"] == "mlp_block":
        x2, z = ops.mlp_block(dv(t["x"]), *args)
    else:
        x2, z = ops.block16(dv(t["o"], dn), dv(t["x"], dn), (dv(t["wp"], dn), dv(t["bp"])), *args)
    vr.check(case, dict(x2=x2, z=z[vr.mlp_kept(p["M"]).to(DEV)]), "%s[%s]" % (p["op"], dn))


PREP = vr.prep_cases()


@pytest.mark.parametrize("case", PREP, ids=ids(PREP))
def test_qkv_prep_with_the_folded_first_layernorm(ops, case):
    t, _, _ = vr.evaluate(case)
    C, k = vr.PREP[3], vr.PREP[4]
    flat = lambda w_, n: dv(w_.reshape(C, n).t().contiguous())
    x = dv(t["x"])
    qq, kk, vv = ops.qkv_prep(x, flat(t["w3"], 9), dv(t["g0"]), dv(t["b0"]), x, x, flat(t["wk"], k * k), flat(t["wv"], k * k),
                              dv(t["g1"]), dv(t["b1"]), dv(t["g2"]), dv(t["b2"]), k, pre_ln=(dv(t["g3"]), dv(t["b3"]), 1e-5, True))
    vr.check(case, dict(q=qq, k=kk, v=vv), "qkv_prep")


WINO_RES = (2, 12, 20, 96, 96)           # the smallest RES_CASES entry of tests/test_gpu_wino.py


@pytest.mark.parametrize("R", [0, 8, 64, 512, "const3", "zero"])
def test_gn_affine_from_the_producers_sums(ops, tuning, R):
    """The F(4x4) convolution leaves per-(image, group) sums of its own output for the next GroupNorm (no pivot is known before the
    convolution runs).  Its bias is R o (o = +-1 by group), so the output carries the offset; x a + b, formed in fp64 from the rows
    of gn_affine_from_stats, against the fp64 GroupNorm of the output the kernel produced.  const3 / zero (part D): zero weights and
    a bias of 3 or 0, a constant output."""
    N, H, W, Cin, Cout = WINO_RES
    tuning.set("DIFFSAL_FORCE_WINOGRAD", 1)
    x = dv(vr.rnd("vr.wx", N, H, W, Cin) * 1.3 + 0.2)
    w1 = vr.rnd("vr.ww1", Cout, Cin, 3, 3, scale=0.05)
    g, b = vr.affine("vr.wgn", Cout)
    if R in vr.FILLS:                                                  # part D: zero weights, the output is the bias everywhere
        w1, bias = torch.zeros_like(w1), torch.full((Cout,), 3.0 if R == "const3" else 0.0)
    else:
        bias = float(R) * vr._alt(32).repeat_interleave(Cout // 32)
    plan = ops.resblock_wino4_plan(x, Cout, 32)
    assert plan is not None and plan["stats"]
    h, _, st = ops.conv3x3_wino4_ex(x, ops.pack_wino4_weight(dv(w1)), bias=dv(bias), stats_groups=32)
    ab = ops.gn_affine_from_stats(st, dv(g), dv(b), vr.GN_EPS).double().cpu()
    hc = h.cpu()
    if R in vr.FILLS:
        assert torch.equal(hc, bias.expand_as(hc))
    case = vr.Case("gn_affine_from_stats-%s" % vr._rs(R), "gn", dict(shape=tuple(hc.shape), R=R, dname="fp32", swish=False, gain=1.0))
    t = dict(x=hc, g=g, b=b)
    ref64, ref32 = vr.gn_reference(case.p, t, torch.float64), vr.gn_reference(case.p, t, torch.float32)
    (m64, d32), = vr.reference_spread(ref64, ref32).values()
    assert 8.0 * d32 <= vr.REF_CAP * m64
    y = hc.double() * ab[:, 0][:, None, None, :] + ab[:, 1][:, None, None, :]
    vr.check(case, dict(y=y), "gn_affine_from_stats", ref64, ref32)


def test_winograd_f4_swish_on_load_sweep(ops, tuning):
    """swishf_fast in the F(4x4) input transform: centre-tap identity weights, affine rows with scale 32 and shift 0, x = s / 32, so
    that the transform's swish sees the swept values s.  The Winograd transforms multiply by up to 8 and cancel, so the sweep stops
    at |s| = 104 here; bound: that path's 1e-4 of max|ref| (tests/test_gpu_wino.py) plus the swish bound."""
    N, H, W, Cin, Cout = 3, 5, 6, 96, 100                              # the smallest CASES4 entry
    tuning.set("DIFFSAL_FORCE_WINOGRAD", 1)
    s = vr.sweep_sample(N * H * W * Cin + 8)
    s = s[s.abs() <= 104.0][:N * H * W * Cin].reshape(N, H, W, Cin)
    x = s / 32.0
    seen = x * 32.0                                                    # what the transform's affine forms (a subnormal loses bits in x)
    w = torch.zeros(Cout, Cin, 3, 3)
    w[torch.arange(Cin), torch.arange(Cin), 1, 1] = 1.0
    ab = torch.stack([torch.full((N, Cin), 32.0), torch.zeros(N, Cin)], 1).contiguous()
    out, _, _ = ops.conv3x3_wino4_ex(dv(x), ops.pack_wino4_weight(dv(w)), gn_ab=dv(ab))
    assert torch.equal(out[..., Cin:], torch.zeros_like(out[..., Cin:]))
    ref = vr.act_ref(seen, "swish")
    vr.act_check(out[..., :Cin], seen, "swish", "F(4x4) swish on load", extra=1e-4 * abs(ref).max())


# ------------------------------------------------------------------------------------------------------------------------
# C: activations over their whole range
# ------------------------------------------------------------------------------------------------------------------------
def eye(n, dname="fp32"):
    return torch.eye(n, device=DEV, dtype=vr.DTYPES[dname])


LINEAR_ROUTES = [
    # name, storage, switches, expected kernel, rows x width the sweep is fed as
    ("igemm", "fp32", {"DIFFSAL_GEMM_DMA": 0, "DIFFSAL_NO_PERSIST": 1}, "igemm_kernel<", 96),
    ("persistent", "fp32", {"DIFFSAL_GEMM_DMA": 0, "DIFFSAL_NO_PERSIST": 0}, "igemm_linear_kernel<", 96),
    ("gemm_dma-1", "fp32", {"DIFFSAL_GEMM_DMA": 1}, "gemm_dma_kernel<float", 96),
    ("gemm_dma-2", "fp32", {"DIFFSAL_GEMM_DMA": 2}, "gemm_dma_kernel<float", 192),    # six stages: K / 32 a multiple of 6
    ("lin_stream", "fp32", {}, "lin_stream_kernel", 96),
    ("igemm16", "bf16", {"DIFFSAL_GEMM_DMA16": 0}, "igemm16", 96),
    ("igemm16", "fp16", {"DIFFSAL_GEMM_DMA16": 0}, "igemm16", 96),
    ("gemm16_dma2", "bf16", {"DIFFSAL_GEMM_DMA16": 3}, "gemm16_dma2_kernel<", 192),      # that kernel takes K in multiples of 192
    ("gemm16_dma2", "fp16", {"DIFFSAL_GEMM_DMA16": 3}, "gemm16_dma2_kernel<", 192),
]


@pytest.mark.parametrize("act", ["gelu", "sigmoid"])
@pytest.mark.parametrize("route", LINEAR_ROUTES, ids=["%s-%s" % r[:2] for r in LINEAR_ROUTES])
def test_linear_epilogue_activation_sweep(ops, tuning, route, act):
    """Identity weight, no bias: the accumulators are the swept values exactly, the epilogue's activation sees each of them.
    lin_stream starts at 65536 rows: the sweep is repeated 96 times and every copy checked."""
    name, dn, switches, kernel, width = route
    for k, v in switches.items():
        tuning.set(k, v)
    x = vr.sweep(dn).reshape(-1, width)
    reps = 96 if name == "lin_stream" else 1
    got = ops.linear(dv(x, dn).repeat(reps, 1), eye(width, dn), None, act=ops.ACT_GELU if act == "gelu" else ops.ACT_SIGMOID)
    assert kernel in last_kernel(), last_kernel()
    got = got.float().reshape(reps, *x.shape)
    assert torch.equal(got, got[:1].expand_as(got))
    vr.act_check(got[0], x, act, "linear[%s,%s]" % (name, dn), u=vr.UNIT[dn], extra=vr.TINY16[dn])


@pytest.mark.parametrize("route", ["tiled", "dma"])
def test_gelu_grad_epilogue_sweep(ops, agops, tuning, route):
    """y = gelu(h) I: the data-gradient product's epilogue multiplies dy I by gelu'(h)"""
    tuning.set("DIFFSAL_GEMM_DMA", 0 if route == "tiled" else 1)
    h = dv(vr.sweep()).requires_grad_(True)
    y = agops.linear(h, eye(96), None, in_gelu=True)
    y.backward(torch.ones_like(y))                                    # the weight is a constant: the data-gradient product is the last launch
    assert ("igemm_" if route == "tiled" else "gemm_dma_kernel<float") in last_kernel(), last_kernel()
    vr.act_check(y, vr.sweep(), "gelu", "autograd linear(in_gelu)[%s] forward" % route)
    vr.act_check(h.grad, vr.sweep(), "gelu_grad", "autograd linear(in_gelu)[%s] backward" % route)


def test_act_bwd_every_mode_sweep(ops):
    x = vr.sweep()
    one = torch.ones_like(x).to(DEV)
    vr.act_check(ops.act_bwd(one, dv(x), 2), x, "gelu_grad", "act_bwd[gelu]")
    got = ops.act_bwd(dv(vr.rnd("vr.abdy", *x.shape)), dv(x), 1).cpu()          # ReLU: ref = y; exact
    assert torch.equal(got, torch.where(x > 0, vr.rnd("vr.abdy", *x.shape), torch.zeros(())))
    y = torch.sigmoid(x.double()).float()                                        # sigmoid: ref = y, dy y (1 - y): three roundings
    got = ops.act_bwd(one, dv(y), 3).double().cpu()
    ref = y.double() * (1.0 - y.double())
    assert ((got - ref).abs() <= 3 * 2.0 ** -24 * ref + 1.2e-38).all()


def test_affine_act_gelu_swish_relu_sweep(ops, agops):
    x = vr.sweep()
    one, zero = torch.ones(1, 96, device=DEV), torch.zeros(1, 96, device=DEV)
    vr.act_check(ops.affine_act(dv(x), one, zero, x.shape[0], 4), x, "swish", "affine_act[swish]")
    vr.act_check(ops.affine_act(dv(x), one, zero, x.shape[0], ops.ACT_RELU), x, "relu", "affine_act[relu]")
    xd = dv(x).requires_grad_(True)
    y = agops.gelu(xd)
    y.backward(torch.ones_like(y))
    vr.act_check(y, x, "gelu", "autograd gelu forward")
    vr.act_check(xd.grad, x, "gelu_grad", "autograd gelu backward")


def test_sigmoid_gate_and_head_sigmoid_sweep(ops):
    x = vr.sweep()
    vr.act_check(ops.sigmoid_gate(dv(x), torch.ones_like(x).to(DEV)), x, "sigmoid", "sigmoid_gate")
    w = torch.zeros(96)
    w[37] = 1.0                                                        # one-hot: the head's sum is channel 37 of each pixel
    xs = torch.zeros(1, x.numel() // 96, 96, 96)
    xs[..., 37] = x.reshape(1, -1, 96)
    got = ops.head_sigmoid(dv(xs), dv(w), torch.zeros(1, device=DEV))
    vr.act_check(got.reshape(x.shape), x, "sigmoid", "head_sigmoid")


@pytest.mark.parametrize("B", [4, 32])
def test_dense_small_and_temb_mlp_swish_sweep(ops, B):
    """identity-like weights: B = 4 takes the row form, B = 32 the lane-per-clip form"""
    x = vr.sweep_sample(B * 96).reshape(B, 96)
    vr.act_check(ops.dense_small(dv(x), eye(96), None, True), x, "swish", "dense_small[B=%d]" % B)
    ch = 96
    b0 = vr.sweep_sample(4 * ch)                                       # hidden = swish(0 + b0), temb = hidden I
    freq = torch.exp(torch.arange(ch // 2, dtype=torch.float32) * -(math.log(10000) / (ch // 2 - 1)))
    got = ops.temb_mlp(torch.arange(B, dtype=torch.float32, device=DEV), dv(freq), torch.zeros(4 * ch, ch, device=DEV), dv(b0),
                       eye(4 * ch), torch.zeros(4 * ch, device=DEV))
    vr.act_check(got, b0.expand(B, -1), "swish", "temb_mlp[B=%d]" % B)


def _formula(x, what):
    """torch's value of the defining formula at +-inf and NaN, in fp64 (IEEE: inf 0 = NaN)"""
    x = x.double()
    if what == "gelu":
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if what == "gelu_grad":
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if what == "swish":
        return x * torch.sigmoid(x)
    raise KeyError(what)


def test_specials_through_the_elementwise_entries(ops, agops):
    """+-inf and NaN: torch's value element by element, every neighbour untouched"""
    x = vr.specials_tensor()
    sp = ~torch.isfinite(x)
    plain = torch.full_like(x, 1.5)
    one, zero = torch.ones(1, 96, device=DEV), torch.zeros(1, 96, device=DEV)
    dy = torch.full_like(x, 2.0)

    def expect(got, ref_special, clean, what):
        """the special places carry torch's value; everywhere else the result is bit for bit the one of the all-1.5 input"""
        g = got.detach().float().cpu()
        assert vr.same_values(g[sp], ref_special.float()[sp]), (what, g[sp].tolist(), ref_special.float()[sp].tolist())
        assert torch.equal(g[~sp], clean.detach().float().cpu()[~sp]), what

    expect(ops.affine_act(dv(x), one, zero, 8, ops.ACT_RELU), F.relu(x), ops.affine_act(dv(plain), one, zero, 8, ops.ACT_RELU), "relu")
    expect(ops.affine_act(dv(x), one, zero, 8, 4), _formula(x, "swish"), ops.affine_act(dv(plain), one, zero, 8, 4), "swish")
    expect(ops.sigmoid_gate(dv(x), dv(dy)), torch.sigmoid(x) * dy, ops.sigmoid_gate(dv(plain), dv(dy)), "sigmoid_gate")
    xd, pd = dv(x).requires_grad_(True), dv(plain).requires_grad_(True)
    y, yp = agops.gelu(xd), agops.gelu(pd)
    y.backward(dv(dy))
    yp.backward(dv(dy))
    expect(y, _formula(x, "gelu"), yp, "gelu")
    expect(xd.grad, 2.0 * _formula(x, "gelu_grad"), pd.grad, "gelu backward")
    expect(ops.act_bwd(dv(dy), dv(x), 1), torch.ops.aten.threshold_backward(dy, x, 0), ops.act_bwd(dv(dy), dv(plain), 1), "act_bwd relu")
    expect(ops.act_bwd(dv(dy), dv(x), 2), 2.0 * _formula(x, "gelu_grad"), ops.act_bwd(dv(dy), dv(plain), 2), "act_bwd gelu")
    expect(ops.act_bwd(dv(dy), dv(x), 3), torch.ops.aten.sigmoid_backward(dy, x), ops.act_bwd(dv(dy), dv(plain), 3), "act_bwd sigmoid")
