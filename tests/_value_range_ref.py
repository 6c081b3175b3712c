"""Inputs, fp64 references and tolerances of the value-range tests (tests/test_value_range_host.py, tests/test_gpu_value_range.py).

Every other GPU test draws its inputs from ``oracle.synth_tensor``: a standard normal times a scale near 1.  The cases here leave
that range: rows whose mean is large against their spread, constant rows, attention logits of several hundred, and activations
over [-40, 40] plus the edges of the float range.  Everything in this module is plain torch / numpy on the CPU.

The rule of parts A, B and D, for an output with fp64 reference ``ref64`` and fp32 torch reference ``ref32`` (both on the exact
values the kernel receives, i.e. already rounded to the storage type):

    max|got - ref64| <= max(T_op * max|ref64|, 8 * max|ref32 - ref64|) + u * max|ref64|

T_op is the tolerance the operation's existing test uses, u the unit roundoff of one final rounding to 16-bit storage.  The factor
8 covers another summation order and the hardware exp / rcp; it does not cover another dependence on the mean offset or on the
size of a logit."""
import collections
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import salunet_oracle as orc

T_FWD = 2e-5                                   # fp32 forward kernels (tests/test_gpu_ops.py)
T_GRAD = 5e-5                                  # GroupNorm / BatchNorm / attention gradients (tests/test_gpu_train_ops.py)
T_RUN = 1e-5                                   # BatchNorm running statistics (tests/test_gpu_train_ops.py)
OP_RTOL = {"bf16": 6e-3, "fp16": 8e-4}         # 16-bit storage, per operator (tests/test_gpu_lowp.py)
UNIT = {"fp32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
REF_CAP = 1e-2                                 # 8 * max|ref32 - ref64| above this share of max|ref64|: not a valid case

Case = collections.namedtuple("Case", "id family p")


def rnd(name, *shape, scale=1.0):
    return orc.synth_tensor(name, shape, scale)


def q(x, dname):
    """round to the storage type and back: the exact values the kernel sees"""
    return x.to(DTYPES[dname]).float()


def leaf(t, dt):
    """a fresh leaf: the cached inputs are shared between tests and never take part in a graph"""
    return t.detach().to(dt).clone().requires_grad_(True)


def t_fwd(dname):
    return T_FWD if dname == "fp32" else OP_RTOL[dname]


# ------------------------------------------------------------------------------------------------------------------------
# part A / D: normalisation under a mean offset, constant rows
# ------------------------------------------------------------------------------------------------------------------------
R_OF = {"fp32": (0, 8, 64, 512), "bf16": (0, 8), "fp16": (0, 8, 64)}
FILLS = ("const3", "zero")                     # part D: value 3.0 (every partial sum is exact) and all-zero rows
GN_SHAPES = [(2, 14, 24, 96), (2, 9, 7, 192), (1, 56, 96, 96), (4, 14, 24, 96)]     # the last: B * groups = 128, the slab's own floor
GN_EPS, LN_EPS, BN_EPS = 1e-6, 1e-5, 1e-5


def _alt(n):
    return torch.where(torch.arange(n) % 2 == 0, 1.0, -1.0)


def offset_input(name, shape, R, by, dname="fp32", groups=32):
    """x = z + R o with o = +-1 alternating by group (NHWC), by row or by channel ([rows, C]); R = 'const3' / 'zero': constant rows."""
    if R == "const3":
        return torch.full(shape, 3.0)
    if R == "zero":
        return torch.zeros(shape)
    z = rnd(name, *shape)
    C = shape[-1]
    if by == "group":
        o = _alt(groups).repeat_interleave(C // groups)
    elif by == "channel":
        o = _alt(C)
    else:
        o = _alt(int(np.prod(shape[:-1]))).reshape(*shape[:-1], 1)
    return q(z + float(R) * o, dname)


def affine(name, C, gain=1.0):
    """gamma = gain (1 + 0.2 z), beta = 0.2 z"""
    return gain * (1.0 + rnd(name + ".g", C, scale=0.2)), rnd(name + ".b", C, scale=0.2)


def _rs(R):
    return R if isinstance(R, str) else "R%d" % R


def gn_cases():
    out = []
    for dname in DTYPES:
        for shape in (GN_SHAPES if dname == "fp32" else GN_SHAPES[:2] + GN_SHAPES[3:]):
            for R in R_OF[dname] + (FILLS if shape == GN_SHAPES[0] or shape == GN_SHAPES[3] else ()):
                out.append(Case("gn_swish-%s-%s-%s" % (dname, "x".join(map(str, shape)), _rs(R)), "gn",
                                dict(shape=shape, R=R, dname=dname, swish=True, gain=1.0)))
    for swish in (True, False):                                       # the legacy U-Net entry
        for R in R_OF["fp32"] + FILLS:
            out.append(Case("gn_legacy-swish%d-%s" % (swish, _rs(R)), "gn",
                            dict(shape=GN_SHAPES[0], R=R, dname="fp32", swish=swish, gain=1.0)))
    return out


def gn_gain_cases():
    """part C: gamma = 32 (1 + 0.2 z), so that swish sees about +-120"""
    return [Case("gn_swish-gain32-%s" % "x".join(map(str, s)), "gn", dict(shape=s, R=0, dname="fp32", swish=True, gain=32.0))
            for s in (GN_SHAPES[0], GN_SHAPES[3])]


def gn_inputs(p):
    C = p["shape"][-1]
    g, b = affine("vr.gn%d" % C, C, p["gain"])
    return dict(x=offset_input("vr.gnx" + "x".join(map(str, p["shape"])), p["shape"], p["R"], "group", p["dname"]), g=g, b=b)


def gn_reference(p, t, dt):
    y = F.group_norm(t["x"].to(dt).permute(0, 3, 1, 2).contiguous(), 32, t["g"].to(dt), t["b"].to(dt), GN_EPS)
    return dict(y=(F.silu(y) if p["swish"] else y).permute(0, 2, 3, 1))


def gn_train_cases():
    return [Case("gn_train-%s" % _rs(R), "gn_train", dict(shape=GN_SHAPES[0], R=R)) for R in R_OF["fp32"] + FILLS]


def gn_train_inputs(p):
    t = gn_inputs(dict(p, dname="fp32", gain=1.0))
    t["dy"] = rnd("vr.gndy", *p["shape"])
    return t


def gn_train_reference(p, t, dt):
    x, g, b = (leaf(t[k], dt) for k in ("x", "g", "b"))
    y = F.silu(F.group_norm(x.permute(0, 3, 1, 2).contiguous(), 32, g, b, GN_EPS)).permute(0, 2, 3, 1)
    y.backward(t["dy"].to(dt))
    return dict(y=y.detach(), dx=x.grad, dgamma=g.grad, dbeta=b.grad)


BN_ROWS, BN_C = 3000, 64


def bn_cases():
    return [Case("bn_train-relu%d-%s" % (relu, _rs(R)), "bn", dict(R=R, relu=relu)) for relu in (True, False)
            for R in R_OF["fp32"] + FILLS]


def bn_inputs(p):
    g, b = affine("vr.bn", BN_C)
    t = dict(x=offset_input("vr.bnx", (BN_ROWS, BN_C), p["R"], "channel"), g=g, b=b, dy=rnd("vr.bndy", BN_ROWS, BN_C),
             rm=rnd("vr.bnrm", BN_C, scale=0.1), rv=rnd("vr.bnrv", BN_C).abs() * 0.3 + 0.7)
    if p["relu"]:
        # ReLU's derivative jumps at 0: an element whose pre-activation lies within rounding of 0 gets another gradient in fp32
        # than in fp64 and the reference itself falls apart (at R = 64 already).  Such elements receive no gradient here.
        pre = F.batch_norm(t["x"].double(), None, None, g.double(), b.double(), True, 0.1, BN_EPS)
        t["dy"] = torch.where(pre.abs() < 2e-3, torch.zeros(()), t["dy"])
    return t


def bn_reference(p, t, dt):
    x, g, b = (leaf(t[k], dt) for k in ("x", "g", "b"))
    rm, rv = t["rm"].to(dt).clone(), t["rv"].to(dt).clone()
    y = F.batch_norm(x, rm, rv, g, b, True, 0.1, BN_EPS)
    y = F.relu(y) if p["relu"] else y
    y.backward(t["dy"].to(dt))
    return dict(y=y.detach(), running_mean=rm, running_var=rv, dx=x.grad, dgamma=g.grad, dbeta=b.grad)


LN_M = 77


def ln_cases():
    out = []
    for C in (32, 96, 768):
        for R in R_OF["fp32"] + FILLS:
            out.append(Case("layernorm-fp32-%dx%d-%s" % (LN_M, C, _rs(R)), "ln", dict(shape=(LN_M, C), R=R, dname="fp32")))
    for dname in ("bf16", "fp16"):                                    # the 16-byte form
        for R in R_OF[dname] + FILLS:
            out.append(Case("layernorm-%s-777x192-%s" % (dname, _rs(R)), "ln", dict(shape=(777, 192), R=R, dname=dname)))
    return out


def ln_inputs(p):
    M, C = p["shape"]
    g, b = affine("vr.ln%d" % C, C, p.get("gain", 1.0))
    return dict(x=offset_input("vr.lnx%dx%d" % (M, C), (M, C), p["R"], "row", p["dname"]), g=g, b=b)


def ln_reference(p, t, dt):
    C = p["shape"][1]
    return dict(y=F.layer_norm(t["x"].to(dt), (C,), t["g"].to(dt), t["b"].to(dt), LN_EPS))


LN_MULTI_ROWS = (77, 5, 130)


def ln_multi_cases():
    return [Case("layernorm_multi-%s" % _rs(R), "ln_multi", dict(R=R)) for R in R_OF["fp32"] + FILLS]


def ln_multi_inputs(p):
    t = {}
    for i, M in enumerate(LN_MULTI_ROWS):
        t["x%d" % i] = offset_input("vr.lmx%d" % i, (M, 96), p["R"], "row")
        t["g%d" % i], t["b%d" % i] = affine("vr.lm%d" % i, 96)
    return t


def ln_multi_reference(p, t, dt):
    return {"y%d" % i: F.layer_norm(t["x%d" % i].to(dt), (96,), t["g%d" % i].to(dt), t["b%d" % i].to(dt), LN_EPS)
            for i in range(len(LN_MULTI_ROWS))}


def ln_bwd_cases():
    return [Case("layernorm_%s-%s" % (form, _rs(R)), "ln_bwd", dict(R=R, fork=form == "fork"))
            for form in ("bwd", "fork") for R in R_OF["fp32"] + FILLS]


def ln_bwd_inputs(p):
    t = ln_inputs(dict(shape=(LN_M, 96), R=p["R"], dname="fp32"))
    t["dy"] = rnd("vr.lndy", LN_M, 96)
    return t


def ln_bwd_reference(p, t, dt):
    """fork: the residual path carries 1.5 x beside the branch (tests/test_gpu_train_ops.py)"""
    x, g, b = (leaf(t[k], dt) for k in ("x", "g", "b"))
    y = F.layer_norm(x, (96,), g, b, LN_EPS)
    (y + 1.5 * x if p["fork"] else y).backward(t["dy"].to(dt))
    return dict(dx=x.grad, dgamma=g.grad, dbeta=b.grad)


# ------------------------------------------------------------------------------------------------------------------------
# part B: softmax with peaked, shifted and flat logits
# ------------------------------------------------------------------------------------------------------------------------
SOFTMAX_MODES = ("a1", "a16", "a128", "flat", "onehot")


def _gain(mode):
    return float(mode[1:]) if mode[0] == "a" else 1.0


def shape_qkv(qq, kk, vv, mode):
    """queries times a; 'flat': all keys equal (the output is the mean of v); 'onehot': key 0 = 20 x query row 0"""
    qq = qq * _gain(mode)
    if mode == "flat":
        kk = kk[..., :1, :].expand_as(kk).contiguous()
    elif mode == "onehot":
        kk = kk.clone()
        kk[..., 0, :] = 20.0 * qq[..., 0, :]
    return qq, kk, vv


ATTN_FP32 = [(96, 200, 18, 2), (32, 64, 2, 2)]                       # C, Lq, Lk, heads (tests/test_gpu_ops.py)
ATTN_16 = [(2, 77, 5, 96, 2), (3, 84, 18, 768, 2)]                   # n, Lq, Lk, C, heads (tests/test_gpu_stream16.py)


def attn_cases():
    out = []
    for C, Lq, Lk, heads in ATTN_FP32:
        for mode in SOFTMAX_MODES:
            out.append(Case("attention-fp32-%d.%d.%d-%s" % (C, Lq, Lk, mode), "attn",
                            dict(n=3, Lq=Lq, Lk=Lk, C=C, heads=heads, dname="fp32", mode=mode)))
    for n, Lq, Lk, C, heads in ATTN_16:
        for dname in ("bf16", "fp16"):
            for mode in SOFTMAX_MODES:
                out.append(Case("attention-%s-%d.%d.%d-%s" % (dname, C, Lq, Lk, mode), "attn",
                                dict(n=n, Lq=Lq, Lk=Lk, C=C, heads=heads, dname=dname, mode=mode)))
    return out


def attn_inputs(p):
    qq, kk, vv = (rnd("vr.a" + nm, p["n"], L, p["C"]) for nm, L in (("q", p["Lq"]), ("k", p["Lk"]), ("v", p["Lk"])))
    qq, kk, vv = shape_qkv(qq, kk, vv, p["mode"])
    return dict(q=q(qq, p["dname"]), k=q(kk, p["dname"]), v=q(vv, p["dname"]))


def _attn(qq, kk, vv, heads, scale):
    n, Lq, C = qq.shape
    d = C // heads
    qh, kh, vh = (t.reshape(n, -1, heads, d).transpose(1, 2) for t in (qq, kk, vv))
    return (F.softmax(qh @ kh.transpose(-1, -2) * scale, -1) @ vh).transpose(1, 2).reshape(n, Lq, C)


def attn_reference(p, t, dt):
    return dict(o=_attn(t["q"].to(dt), t["k"].to(dt), t["v"].to(dt), p["heads"], p["C"] ** -0.5))


def attn_bwd_cases():
    C, Lq, Lk, heads = ATTN_FP32[0]
    return [Case("attention_bwd-%s" % mode, "attn_bwd", dict(n=3, Lq=Lq, Lk=Lk, C=C, heads=heads, dname="fp32", mode=mode))
            for mode in SOFTMAX_MODES]


def attn_bwd_inputs(p):
    t = attn_inputs(p)
    t["do"] = rnd("vr.ado", p["n"], p["Lq"], p["C"])
    return t


def attn_bwd_reference(p, t, dt):
    qq, kk, vv = (leaf(t[k], dt) for k in "qkv")
    _attn(qq, kk, vv, p["heads"], p["C"] ** -0.5).backward(t["do"].to(dt))
    return dict(dq=qq.grad, dk=kk.grad, dv=vv.grad)


ATTN_GENERAL = [(2, 2, 150, 70, 64, 0), (1, 2, 121, 31, 96, 48)]     # B, H, Lq, Lk, D, E (tests/test_gpu_encoder_train.py)


def attn_general_cases():
    return [Case("attention_general-%d.%d.E%d-%s" % (s[2], s[3], s[5], mode), "attn_general", dict(shape=s, mode=mode))
            for s in ATTN_GENERAL for mode in SOFTMAX_MODES]


def attn_general_inputs(p):
    B, H, Lq, Lk, D, E = p["shape"]
    qq, kk, vv = (rnd("vr.g" + nm, B, H, L, D) for nm, L in (("q", Lq), ("k", Lk), ("v", Lk)))
    qq, kk, vv = shape_qkv(qq, kk, vv, p["mode"])
    t = dict(q=qq, k=kk, v=vv, do=rnd("vr.gdo", B, Lq, H * D))
    if E:
        t["qe"] = rnd("vr.gqe", B, H, Lq, E, scale=0.3) * _gain(p["mode"])
        ke = torch.zeros(Lk, E)
        ke[torch.arange(1, Lk), torch.randint(0, E, (Lk - 1,), generator=torch.Generator().manual_seed(1))] = 1.0
        t["ke"] = ke
    return t


def attn_general_reference(p, t, dt):
    """the dense formula of tests/test_gpu_encoder_train.py; with E: relative-position term, residual on rows 1.. (skip_first)"""
    B, H, Lq, Lk, D, E = p["shape"]
    qq, kk, vv = (leaf(t[k], dt) for k in "qkv")
    s = (qq * D ** -0.5) @ kk.transpose(-1, -2)
    qe = None
    if E:
        qe = leaf(t["qe"], dt)
        s = s + qe @ t["ke"].to(dt).t()
    o = s.softmax(-1) @ vv
    if E:
        o = torch.cat([o[:, :, :1], o[:, :, 1:] + qq[:, :, 1:]], 2)
    o = o.transpose(1, 2).reshape(B, Lq, H * D)
    (o * t["do"].to(dt)).sum().backward()
    r = dict(o=o.detach(), lse=torch.logsumexp(s.detach(), -1), dq=qq.grad, dk=kk.grad, dv=vv.grad)
    if E:
        r["dqe"] = qe.grad
    return r


SOFTMAX_ROWS = [(333, 18), (64, 673)]


def softmax_cases():
    return [Case("softmax_rows-%dx%d-%s" % (r, c, mode), "softmax", dict(rows=r, cols=c, mode=mode))
            for r, c in SOFTMAX_ROWS for mode in SOFTMAX_MODES]


def softmax_inputs(p):
    """logits 0.7 a z; 'flat': every column equal; 'onehot': column 0 stands 60 above the rest (after the scale)"""
    x = rnd("vr.sm", p["rows"], p["cols"]) * _gain(p["mode"])
    if p["mode"] == "flat":
        x = x[:, :1].expand_as(x).contiguous()
    elif p["mode"] == "onehot":
        x[:, 0] += 60.0 / 0.7
    return dict(x=x)


def softmax_reference(p, t, dt):
    return dict(y=F.softmax(t["x"].to(dt) * 0.7, -1))


ATTN_FOLD = [(384, 8, 2), (192, 333, 18)]                            # C, L, Lk (tests/test_gpu_attn_fold.py)


def attn_fold_cases():
    return [Case("attn_fold-%d.%d.%d-%s" % (C, L, Lk, mode), "attn_fold", dict(C=C, L=L, Lk=Lk, mode=mode))
            for C, L, Lk in ATTN_FOLD for mode in SOFTMAX_MODES]


def attn_fold_inputs(p):
    from tests.test_gpu_attn_fold import _problem

    t, w, b = _problem(p["C"], p["L"], p["Lk"], 3, tag="vr")
    t, b = attn_fold_shape_inputs(t, w, b, p["mode"])
    return dict(t=t, w=w, b=b)


def attn_fold_shape_inputs(t, w, b, mode):
    """The query of the fold is qin Wq^T + bq and its key kp Wk^T + bk: the gain goes on qin and bq; 'flat' repeats the pooled
    key row; 'onehot' solves for the pooled row 0 whose PROJECTED key is twenty times the projected query 0."""
    t, b = dict(t), dict(b)
    a = _gain(mode)
    t["qin"], b["q"] = t["qin"] * a, b["q"] * a
    if mode == "flat":
        t["kp"] = t["kp"][:, :1].expand_as(t["kp"]).contiguous()
    elif mode == "onehot":
        qp = t["qin"][:, 0].double() @ w["q"].double().T + b["q"].double()
        kp0 = torch.linalg.solve(w["k"].double(), (20.0 * qp - b["k"].double()).T).T
        t["kp"] = t["kp"].clone()
        t["kp"][:, 0] = kp0.float()
    return t, b


def attn_fold_reference(p, inp, dt, heads=2):
    """q -> softmax -> o -> proj + residual (tests/test_gpu_attn_fold.py), in the given precision"""
    t, w, b = inp["t"], inp["w"], inp["b"]
    td, wd, bd = ({k: v.to(dt) for k, v in s.items()} for s in (t, w, b))
    n, L, C = td["qin"].shape
    qq = td["qin"] @ wd["q"].T + bd["q"]
    kk = td["kp"] @ wd["k"].T + bd["k"]
    vv = td["vp"] @ wd["v"].T + bd["v"]
    return dict(y=_attn(qq, kk, vv, heads, C ** -0.5) @ wd["p"].T + bd["p"] + td["x"])


# ------------------------------------------------------------------------------------------------------------------------
# the LayerNorms and the softmax inside the fused blocks (builders of the blocks' own tests, references restated for any precision)
# ------------------------------------------------------------------------------------------------------------------------
FRONT_A, FRONT_B = (2, 8, 16, 2), (2, 13, 21, 18)                    # N, H, W, Lk at C = 96 (tests/test_gpu_block_front_fold.py)


def front_cases():
    return ([Case("block_front-%s" % _rs(R), "front", dict(shape=FRONT_A, R=R, mode="a1")) for R in R_OF["fp32"] + FILLS]
            + [Case("block_front-%s" % mode, "front", dict(shape=FRONT_B, R=0, mode=mode)) for mode in SOFTMAX_MODES])


def _front_q(x, prm, w, b, dt):
    """LayerNorm -> depthwise 3x3 -> LayerNorm -> proj_q: the query of the block front, [N, HW, C]"""
    N, H, W, C = x.shape
    prm, w, b = ({k: v.to(dt) for k, v in s_.items()} for s_ in (prm, w, b))
    xn = F.layer_norm(x.to(dt), (C,), prm["g1"], prm["b1"], LN_EPS)
    qd = F.conv2d(xn.permute(0, 3, 1, 2), prm["w9"].t().reshape(C, 1, 3, 3), None, padding=1, groups=C).permute(0, 2, 3, 1)
    return F.layer_norm(qd, (C,), prm["gq"], prm["bq"], LN_EPS).reshape(N, H * W, C) @ w["q"].T + b["q"]


def front_inputs(p):
    """token rows offset by +-R (alternating by token), or the pooled key rows shaped by the softmax mode (kp times a)"""
    from tests.test_gpu_block_front_fold import _problem

    N, H, W, Lk = p["shape"]
    x, kp, vp, prm, w, b = _problem(N, H, W, Lk, tag="vr")
    if p["R"] in FILLS:
        x = offset_input("", tuple(x.shape), p["R"], "row")
    elif p["R"]:
        x = x + float(p["R"]) * _alt(N * H * W).reshape(N, H, W, 1)
    kp = kp * _gain(p["mode"])
    if p["mode"] == "flat":
        kp = kp[:, :1].expand_as(kp).contiguous()
    elif p["mode"] == "onehot":                                       # the pooled row 0 whose projected key is 20 x the projected query 0
        q0 = _front_q(x, prm, w, b, torch.float64)[:, 0]
        kp = kp.clone()
        kp[:, 0] = torch.linalg.solve(w["k"].double(), (20.0 * q0 - b["k"].double()).T).T.float()
    return dict(x=x, kp=kp, vp=vp, prm=prm, w=w, b=b)


def front_reference(p, t, dt):
    """tests/test_gpu_block_front_fold.py::_reference64 in the given precision"""
    x = t["x"].to(dt)
    N, H, W, C = x.shape
    w, b = ({k: v.to(dt) for k, v in s_.items()} for s_ in (t["w"], t["b"]))
    qq = _front_q(t["x"], t["prm"], t["w"], t["b"], dt)
    kk, vv = t["kp"].to(dt) @ w["k"].T + b["k"], t["vp"].to(dt) @ w["v"].T + b["v"]
    return dict(y=(_attn(qq, kk, vv, 2, float(C) ** -0.5) @ w["p"].T + b["p"]).reshape(N, H, W, C) + x)


MLP_FRAMES = (7, 9, 5)                                               # hw, T, kept frames: the rows of z that are written


def mlp_cases():
    out = []
    for op, M, dnames in (("mlp_block", 64, ("fp32",)), ("block16", 77, ("bf16", "fp16"))):
        for dname in dnames:
            for R in R_OF[dname] + FILLS:
                out.append(Case("%s-%s-%s" % (op, dname, _rs(R)), "mlp", dict(op=op, M=M, dname=dname, R=R, gain=1.0)))
            out.append(Case("%s-%s-gain32" % (op, dname), "mlp", dict(op=op, M=M, dname=dname, R=0, gain=32.0)))
    return out


def mlp_inputs(p):
    """tests/test_gpu_ops.py::test_mlp_block_fused_kernel / tests/test_gpu_lowp.py::test_block16_fused_kernel, token rows offset;
    gain32: the LayerNorm gain at 32, so that GELU sees about +-100 (part C)"""
    C, HID, M, dn = 96, 192, p["M"], p["dname"]
    t = dict(x=offset_input("vr.mbx", (M, C), p["R"], "row", dn), g2=p["gain"] * (rnd("vr.mbg", C, scale=0.1) + 1), b2n=rnd("vr.mbb", C, scale=0.1),
             w1=q(rnd("vr.mbw1", HID, C, scale=0.12), dn), bb1=rnd("vr.mbb1", HID, scale=0.1),
             w2=q(rnd("vr.mbw2", C, HID, scale=0.08), dn), bb2=rnd("vr.mbb2", C, scale=0.1),
             gz=rnd("vr.mbgz", C, scale=0.1) + 1, bz=rnd("vr.mbbz", C, scale=0.1))
    if p["op"] == "block16":
        t.update(o=q(rnd("vr.mbo", M, C), dn), wp=q(rnd("vr.mbwp", C, C, scale=0.1), dn), bp=rnd("vr.mbbp", C, scale=0.1))
    return t


def mlp_kept(M):
    hw, T, keep = MLP_FRAMES
    return ((torch.arange(M) // hw) % T) < keep


def mlp_reference(p, t, dt):
    d = {k: v.to(dt) for k, v in t.items()}
    x1 = d["x"] + F.linear(d["o"], d["wp"], d["bp"]) if p["op"] == "block16" else d["x"]
    x2 = x1 + F.linear(F.gelu(F.linear(F.layer_norm(x1, (96,), d["g2"], d["b2n"], LN_EPS), d["w1"], d["bb1"])), d["w2"], d["bb2"])
    return dict(x2=x2, z=F.layer_norm(x2, (96,), d["gz"], d["bz"], LN_EPS)[mlp_kept(p["M"])])


PREP = (2, 9, 10, 96, 3)                                             # N, H, W, C, k (tests/test_gpu_stream16.py::PREP_CASES, the last)


def prep_cases():
    return [Case("qkv_prep-%s" % _rs(R), "prep", dict(R=R)) for R in R_OF["fp32"] + FILLS]


def prep_inputs(p):
    """the merged query / pooled key / value launch with the block's first LayerNorm folded into its loads; pixels offset by +-R"""
    N, H, W, C, k = PREP
    t = dict(x=offset_input("vr.qpx", (N, H, W, C), p["R"], "row"), w3=rnd("vr.qpw3", C, 1, 3, 3, scale=0.3),
             wk=rnd("vr.qpwk", C, 1, k, k, scale=1.0 / k), wv=rnd("vr.qpwv", C, 1, k, k, scale=1.0 / k))
    for i in range(4):
        t["g%d" % i], t["b%d" % i] = rnd("vr.qpg%d" % i, C, scale=0.2) + 1.0, rnd("vr.qpb%d" % i, C, scale=0.2)
    return t


def prep_reference(p, t, dt):
    N, H, W, C, k = PREP
    d = {k_: v.to(dt) for k_, v in t.items()}
    n = F.layer_norm(d["x"], (C,), d["g3"], d["b3"], LN_EPS).permute(0, 3, 1, 2)
    tok = lambda m: m.flatten(2).transpose(1, 2)
    return dict(q=F.layer_norm(tok(F.conv2d(n, d["w3"], padding=1, groups=C)), (C,), d["g0"], d["b0"], LN_EPS),
                k=F.layer_norm(tok(F.conv2d(n, d["wk"], stride=k, groups=C)), (C,), d["g1"], d["b1"], LN_EPS),
                v=F.layer_norm(tok(F.conv2d(n, d["wv"], stride=k, groups=C)), (C,), d["g2"], d["b2"], LN_EPS))


# ------------------------------------------------------------------------------------------------------------------------
# the rule of parts A, B and D
# ------------------------------------------------------------------------------------------------------------------------
FAMILIES = {
    "gn": (gn_inputs, gn_reference), "gn_train": (gn_train_inputs, gn_train_reference), "bn": (bn_inputs, bn_reference),
    "ln": (ln_inputs, ln_reference), "ln_multi": (ln_multi_inputs, ln_multi_reference), "ln_bwd": (ln_bwd_inputs, ln_bwd_reference),
    "attn": (attn_inputs, attn_reference), "attn_bwd": (attn_bwd_inputs, attn_bwd_reference),
    "attn_general": (attn_general_inputs, attn_general_reference), "softmax": (softmax_inputs, softmax_reference),
    "attn_fold": (attn_fold_inputs, attn_fold_reference), "front": (front_inputs, front_reference), "mlp": (mlp_inputs, mlp_reference), "prep": (prep_inputs, prep_reference),
}


def t_op(case, name):
    dname = case.p.get("dname", "fp32")
    if name.startswith("running"):
        return T_RUN
    if name in ("dx", "dgamma", "dbeta", "dq", "dk", "dv", "dqe") and case.family != "ln_bwd":
        return T_GRAD
    if case.family == "mlp" and dname != "fp32":
        return 3 * OP_RTOL[dname]              # three chained 16-bit products (tests/test_gpu_lowp.py::test_block16_fused_kernel)
    return t_fwd(dname)


def all_cases():
    return (gn_cases() + gn_gain_cases() + gn_train_cases() + bn_cases() + ln_cases() + ln_multi_cases() + ln_bwd_cases()
            + attn_cases() + attn_bwd_cases() + attn_general_cases() + softmax_cases() + attn_fold_cases() + front_cases() + mlp_cases() + prep_cases())


@functools.lru_cache(maxsize=None)
def _evaluate(case_id):
    case = {c.id: c for c in all_cases()}[case_id]
    make, ref = FAMILIES[case.family]
    t = make(case.p)
    return t, ref(case.p, t, torch.float64), ref(case.p, t, torch.float32)


def evaluate(case):
    """-> (inputs, ref64, ref32), computed once per case and shared by every test that needs it: treat as read-only"""
    return _evaluate(case.id)


def is_fill(case):
    return case.p.get("R") in FILLS


GRADS = ("dx", "dgamma", "dbeta")


def outside_the_rule(case):
    """Outputs whose reference does not support the rule, with what is asserted of them instead:
    * gradients through constant rows (x - mean = 0 times 1 / sqrt(eps)): finite;
    * dq with all keys equal and no relative-position term: it is 0 in exact arithmetic (the rows of dS sum to 0 and every key is
      the same), so max|ref64| is rounding noise.  Bound: T_GRAD of the size dq has with the keys as drawn (mode a1)."""
    if is_fill(case) and case.family in ("gn_train", "bn", "ln_bwd"):
        return GRADS
    if case.p.get("mode") == "flat" and (case.family == "attn_bwd" or (case.family == "attn_general" and case.p["shape"][5] == 0)):
        return ("dq",)
    return ()


def flat_dq_bound(case):
    sib = next(c for c in all_cases() if c.family == case.family and c.p == dict(case.p, mode="a1"))
    return T_GRAD * evaluate(sib)[1]["dq"].abs().max().item()


def reference_spread(ref64, ref32):
    """{output: (max|ref64|, max|ref32 - ref64|)}"""
    return {k: (ref64[k].abs().max().item(), (ref32[k].double() - ref64[k]).abs().max().item()) for k in ref64}


def bound(m64, d32, T, u):
    return max(T * m64, 8.0 * d32) + u * m64


def verdict(case, got, ref64=None, ref32=None, only=None):
    """-> [(output, error, bound, ratio to the fp32 reference's own error)] for the outputs in ``got``"""
    if ref64 is None:
        _, ref64, ref32 = evaluate(case)
    u = UNIT[case.p.get("dname", "fp32")]
    rows = []
    out = outside_the_rule(case)
    for k, (m64, d32) in reference_spread(ref64, ref32).items():
        if k not in got or (only is not None and k not in only):
            continue
        g = got[k].detach().double().cpu()
        assert g.shape == ref64[k].shape, (case.id, k, g.shape, ref64[k].shape)
        assert torch.isfinite(g).all(), (case.id, k, "not finite")
        err = (g - ref64[k]).abs().max().item()
        if k in out:
            rows.append((k, err, flat_dq_bound(case) if k == "dq" else math.inf, math.nan))
            continue
        rows.append((k, err, bound(m64, d32, t_op(case, k), u), err / d32 if d32 > 0 else (0.0 if err == 0 else math.inf)))
    return rows


def check(case, got, label, ref64=None, ref32=None, only=None):
    rows = verdict(case, got, ref64, ref32, only)
    assert rows, case.id
    for k, err, bnd, ratio in rows:
        print(f"{label} {case.id} {k}: max|got-ref64| {err:.3e} bound {bnd:.3e} ratio-to-fp32-ref {ratio:.2f}")
    bad = [(k, err, bnd) for k, err, bnd, _ in rows if not err <= bnd]
    assert not bad, (label, case.id, bad)


# ------------------------------------------------------------------------------------------------------------------------
# part C: activations over their whole range
# ------------------------------------------------------------------------------------------------------------------------
SWEEP_SHAPE = (688, 96)
SPLICED = (0.0, 1e-30, 1e-40, 20.0, 87.0, 88.8, 104.0, 1e4, 3e38)


@functools.lru_cache(maxsize=None)
def _sweep():
    n = SWEEP_SHAPE[0] * SWEEP_SHAPE[1]
    x = np.linspace(-40.0, 40.0, n).astype(np.float32)
    sp = np.array([s * v for v in SPLICED for s in (1.0, -1.0)], dtype=np.float32)
    at = (np.arange(len(sp)) * 3671 + 101) % n                       # scattered, so that no two share a 16-byte access
    x[at] = sp
    return torch.from_numpy(x).reshape(SWEEP_SHAPE)


def sweep(dname="fp32"):
    """66048 values [688, 96]: a uniform grid on [-40, 40] with +-0, +-1e-30, +-1e-40 (subnormal), +-20, +-87, +-88.8, +-104, +-1e4,
    +-3e38 spliced in.  16-bit storage: rounded to the type, values beyond its range dropped to its largest finite value."""
    x = _sweep().clone()
    if dname != "fp32":
        big = torch.finfo(DTYPES[dname]).max
        x = q(x.clamp(-big, big), dname)
    return x


def sweep_sample(n):
    """n values of the sweep: every spliced value and an even pick of the grid"""
    flat = _sweep().reshape(-1)
    sp = torch.tensor([s * v for v in SPLICED for s in (1.0, -1.0)], dtype=torch.float32)
    pick = flat[torch.linspace(0, flat.numel() - 1, n - sp.numel()).long()]
    return torch.cat([sp, pick])


TINY16 = {"fp32": 0.0, "bf16": 2.0 ** -134, "fp16": 2.0 ** -25}      # half the smallest subnormal: a rounding to storage near 0


def _erf64(x):
    return np.vectorize(math.erf)(x)


def act_ref(x, act):
    """fp64 reference of act on a float tensor (numpy float64 out)"""
    x = x.double().numpy()
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if act == "gelu":
            return 0.5 * x * (1.0 + _erf64(x / math.sqrt(2.0)))
        if act == "gelu_grad":
            return 0.5 * (1.0 + _erf64(x / math.sqrt(2.0))) + x * np.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        if act == "sigmoid":
            return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))
        if act == "swish":
            return x * act_ref(torch.from_numpy(x), "sigmoid")
        if act == "relu":
            return np.maximum(x, 0.0)
    raise KeyError(act)


POLY_EPS = 1.5e-7                                                     # Abramowitz & Stegun 7.1.26: |erf error| <= 1.5e-7


def act_bound(x, ref, act, u=0.0):
    """Element-wise bound: the stated error of the polynomial plus the one-ulp hardware operations; 16-bit outputs add u |ref|."""
    ax, aref = np.abs(x.double().numpy()), np.abs(ref)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if act == "gelu":
            b = 0.5 * ax * (POLY_EPS + 2.0 ** -22) + 2.0 ** -22 * aref
        elif act == "gelu_grad":
            phi = np.exp(-0.5 * ax * ax) / math.sqrt(2.0 * math.pi)
            b = 0.5 * (POLY_EPS + 2.0 ** -22) + ax * phi * 2.0 ** -21 + 2.0 ** -23
        elif act in ("sigmoid", "swish"):
            b = (4.0 + ax) * 2.0 ** -23 * aref + 1.2e-38
        elif act == "relu":
            b = np.zeros_like(aref)
        else:
            raise KeyError(act)
    return b + u * aref


def act_check(got, x, act, label, u=0.0, extra=0.0):
    """got against the fp64 reference on x under act_bound (+ ``extra``, an absolute term a caller derives for its own kernel);
    prints the worst share of the bound."""
    ref = act_ref(x, act)
    g = got.detach().double().cpu().numpy().reshape(ref.shape)
    assert np.isfinite(g).all(), (label, "not finite at", x.reshape(-1)[np.flatnonzero(~np.isfinite(g).reshape(-1))[:8]].tolist())
    err, b = np.abs(g - ref), act_bound(x, ref, act, u) + extra
    share = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))
    i = int(np.argmax(share))
    xf = x.reshape(-1)
    print(f"{label} {act}: worst share of the bound {share.reshape(-1)[i]:.3f} at x = {xf[i].item():.9g} "
          f"(got {g.reshape(-1)[i]:.9g}, ref {ref.reshape(-1)[i]:.9g})")
    bad = np.flatnonzero((err > b).reshape(-1))
    assert bad.size == 0, (label, act, [(xf[j].item(), g.reshape(-1)[j], ref.reshape(-1)[j]) for j in bad[:8]])


# float32 restatements of the kernels' own forms (csrc/common.h), for the host test: the bounds above are attainable in fp32
def f32_erf_as(x):
    f = np.float32
    ax = np.abs(x)
    t = f(1.0) / (f(0.3275911) * ax + f(1.0))
    p = f(1.061405429) * t + f(-1.453152027)
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = p * t + f(c)
    with np.errstate(over="ignore", under="ignore"):
        r = f(1.0) - p * t * np.exp(-ax * ax)
    return np.copysign(r, x)


def f32_forms(x, act):
    """numpy float32 restatement: libm exp / erf for sigmoid, swish and gelu ('libm'), and the polynomial of erf_as ('poly')"""
    f = np.float32
    x = x.numpy().astype(np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if act == "sigmoid":
            return f(1.0) / (f(1.0) + np.exp(-x))
        if act == "swish_plain":                                      # overflows exp below -88.7: 0 where the value is still normal
            return x / (f(1.0) + np.exp(-x))
        if act == "swish":                                            # e = exp(-|x|): swishf of csrc/common.h
            e = np.exp(-np.abs(x))
            return np.where(x < 0, x * e, x) / (f(1.0) + e)
        if act == "gelu":
            return f(0.5) * x * (f(1.0) + np.vectorize(math.erf)(x.astype(np.float64) * math.sqrt(0.5)).astype(np.float32))
        if act == "gelu_poly":
            return f(0.5) * x * (f(1.0) + f32_erf_as(x * f(0.70710678118654752440)))
        if act == "gelu_grad_poly":
            ax = np.abs(x) * f(0.70710678118654752440)
            e = np.exp(-ax * ax)
            erf_x = f32_erf_as(x * f(0.70710678118654752440))
            return x * f(0.3989422804014327) * e + f(0.5) * (f(1.0) + erf_x)
    raise KeyError(act)


SPECIALS = (float("inf"), float("-inf"), float("nan"))


def specials_tensor():
    """[8, 96] of 1.5 with +inf, -inf and NaN at scattered places, every one with ordinary neighbours inside its 16-byte access"""
    x = torch.full((8, 96), 1.5)
    where = {(1, 5): SPECIALS[0], (2, 50): SPECIALS[1], (4, 95): SPECIALS[2], (6, 0): SPECIALS[2], (7, 33): SPECIALS[0]}
    for (r, c), v in where.items():
        x[r, c] = v
    return x


def same_values(got, ref):
    """element by element: equal where the reference is a number (inf included), NaN where it is NaN"""
    g, r = got.detach().float().cpu(), ref.detach().float().cpu()
    return bool((torch.isnan(g) == torch.isnan(r)).all() and torch.equal(torch.nan_to_num(g, nan=0.0), torch.nan_to_num(r, nan=0.0)))
