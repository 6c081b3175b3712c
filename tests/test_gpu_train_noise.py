"""Device training noise on the GPU (include/diffsal.h "training noise"): the fused prepare launch against the stand-alone launches
and the NumPy restatement, keyed dropout, layout independence of what a sample sees, and exact resume of a training run."""
import numpy as np
import pytest
import torch

from oracle import salunet_oracle as orc
from tests import _philox_ref as ref
from tests._cases import CASES
from tests.test_gpu_salunet import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
IDS6 = [0, 7, (1 << 32) + 5, 1 << 40, 3, 123456789]
T = 1000
DROP_SHAPES = [(56, 96, 192), (28, 48, 384), (14, 24, 768)]       # the model's three dropout tensors, channels-last


def _tables():
    from diff_sal_amd.diffusion_utils import get_beta_schedule, to_torch

    betas = to_torch(get_beta_schedule("cosine", beta_start=1e-4, beta_end=0.02, num_diffusion_timesteps=T))
    a_hat = (1.0 - betas).cumprod(dim=0)
    return torch.sqrt(a_hat), torch.sqrt(1.0 - a_hat)


def _ref_t(seed, step, cid):
    from diff_sal_amd import ops

    w0 = int(ref.bits(seed, [cid], ops.train_draw(step, ops.TRAIN_TIMESTEP), 1)[0, 0])
    return (w0 * T) >> 32


def _sal(B, hw, tag):
    g = torch.Generator().manual_seed(sum(map(ord, tag)))
    return torch.rand((B, 1) + tuple(hw), generator=g).to(DEV)


@pytest.mark.parametrize("mode", ["fixed", "batch", "per_sample"])
@pytest.mark.parametrize("dq", [0.01, 0.0])
@pytest.mark.parametrize("hw", [(7, 9), (64, 128), (224, 384)])
@pytest.mark.parametrize("B", [1, 3, 4])
def test_fused_prepare_equals_the_launches_it_replaces(B, hw, dq, mode):
    """x0, x_t and noise bit-equal to philox_normal (purposes 0, 1) + the two axpbypcz calls of prepare_data."""
    from diff_sal_amd import ops

    seed, step = (3 << 32) | 77, 5
    ids = [11, (1 << 33) + 1, 4, 1 << 41][:B]
    ta, tb = _tables()
    sal = _sal(B, hw, f"prep{B}{hw}")
    key = ops.train_key(seed, step, DEV)
    ids_t = ops.sample_ids(ids, DEV, B)
    t0 = 617 if mode == "fixed" else None
    x0, x_t, t, noise = ops.train_prepare(sal, ids_t, key, ta.to(DEV), tb.to(DEV), dq_scale=dq, t_mode=mode, t0=t0)
    want_t = {"fixed": [617] * B, "batch": [_ref_t(seed, step, ids[0])] * B, "per_sample": [_ref_t(seed, step, i) for i in ids]}[mode]
    assert t.dtype == torch.int64 and t.tolist() == want_t
    z1 = ops.philox_normal(ids, seed, ops.train_draw(step, ops.TRAIN_NOISE), (1,) + hw)
    r_x0 = sal
    if dq != 0.0:
        z0 = ops.philox_normal(ids, seed, ops.train_draw(step, ops.TRAIN_DEQUANT), (1,) + hw)
        r_x0 = ops.axpbypcz(sal, 1.0, z0, dq)
    r_xt = torch.cat([ops.axpbypcz(r_x0[n:n + 1].contiguous(), float(ta[want_t[n]]), z1[n:n + 1].contiguous(), float(tb[want_t[n]]))
                      for n in range(B)])
    assert torch.equal(noise, z1) and torch.equal(x0, r_x0) and torch.equal(x_t, r_xt)
    assert torch.equal(sal, _sal(B, hw, f"prep{B}{hw}"))              # the input is read only
    _, x_t2, _, none = ops.train_prepare(sal, ids_t, key, ta.to(DEV), tb.to(DEV), dq_scale=dq, t_mode=mode, t0=t0, want_noise=False)
    assert none is None and torch.equal(x_t2, x_t)


@pytest.mark.parametrize("hw", [(224, 384), (7, 9)])
@pytest.mark.parametrize("step", [0, 3, (1 << 27) - 1])
def test_prepare_against_the_restatement(hw, step):
    """t is the integer formula on the restatement's words, exactly.  x_t against the fp64 evaluation on the restatement's
    normals, elementwise within 5e-7 (|b| + dq |a|) + 2 ulp(|x_t|): 5e-7 for each of the two normals scaled by its coefficient,
    the ulp term for the fp32 roundings of the two linear combinations."""
    from diff_sal_amd import ops

    seed = (0x9A << 32) | 0x1234567
    ids = [3, (1 << 32) + 5, 1 << 40, (1 << 62) + 9]
    B, per, dq = len(ids), hw[0] * hw[1], 0.01
    ta, tb = _tables()
    sal = _sal(B, hw, f"ref{hw}")
    key = ops.train_key(seed, step, DEV)
    x0, x_t, t, noise = ops.train_prepare(sal, ops.sample_ids(ids, DEV), key, ta.to(DEV), tb.to(DEV), dq_scale=dq, t_mode="per_sample")
    want_t = [_ref_t(seed, step, i) for i in ids]
    assert t.tolist() == want_t and all(0 <= v < T for v in want_t)
    z0 = ref.normals(seed, ids, ops.train_draw(step, ops.TRAIN_DEQUANT), per)
    z1 = ref.normals(seed, ids, ops.train_draw(step, ops.TRAIN_NOISE), per)
    a = ta[want_t].double().numpy()[:, None]
    b = tb[want_t].double().numpy()[:, None]
    s64 = sal.cpu().numpy().reshape(B, per).astype(np.float64)
    want = a * (s64 + np.float64(np.float32(dq)) * z0) + b * z1
    got32 = x_t.cpu().numpy().reshape(B, per)
    err = np.abs(got32.astype(np.float64) - want)
    bound = 5e-7 * (np.abs(b) + dq * np.abs(a)) + 2.0 * np.spacing(np.abs(got32)).astype(np.float64)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"train_prepare {hw} step {step}: t = {want_t}; max |x_t - fp64| = {err.max():.3e}; worst error / bound = "
          f"{(err / bound).max():.3f} at {worst} (err {err[worst]:.3e}, bound {bound[worst]:.3e}, x_t {got32[worst]:.6f})")
    assert (err <= bound).all()
    assert np.abs(noise.cpu().numpy().reshape(B, per) - z1).max() < 2e-5          # the normals' own bar (test_gpu_device_noise.py)


def _keep(seed, step, ids, site, per, p):
    from diff_sal_amd import ops

    thr = int(float(np.float32(p)) * 4294967296.0)
    return ref.bits(seed, ids, ops.train_draw(step, ops.TRAIN_DROPOUT0 + site), per) >= np.uint32(thr)


@pytest.mark.parametrize("site, shape", list(enumerate(DROP_SHAPES)))
def test_keyed_dropout_mask_is_the_restatement_and_the_backward_reapplies_it(site, shape):
    from diff_sal_amd import autograd_ops as ag
    from diff_sal_amd import ops

    seed, step, p = 1234, 2, 0.1
    ids = [5, (1 << 35) + 2]
    B, per = 2, shape[0] * shape[1] * shape[2]
    g = torch.Generator().manual_seed(site)
    x = (torch.rand((B,) + shape, generator=g) + 0.5).to(DEV)
    dy = (torch.rand((B,) + shape, generator=g) + 0.5).to(DEV)
    key, ids_t = ops.train_key(seed, step, DEV), ops.sample_ids(ids, DEV)
    keep = torch.from_numpy(_keep(seed, step, ids, site, per, p)).view((B,) + shape).to(DEV)
    scale = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    out = ops.dropout_keyed(x, p, ids_t, key, site)
    assert torch.equal(out != 0, keep)
    assert torch.equal(out, torch.where(keep, x * scale.to(DEV), torch.zeros_like(x)))
    frac = 1.0 - keep.float().mean().item()
    assert abs(frac - p) < 5 * (p * (1 - p) / keep.numel()) ** 0.5
    xg = x.clone().requires_grad_(True)
    ag.dropout_keyed(xg, p, ids_t, key, site).backward(dy)
    assert torch.equal(xg.grad, torch.where(keep, dy * scale.to(DEV), torch.zeros_like(dy)))
    # another site, step or seed: another mask
    for other in (ops.dropout_keyed(x, p, ids_t, key, (site + 1) % 3),
                  ops.dropout_keyed(x, p, ids_t, ops.train_key(seed, step + 1, DEV), site),
                  ops.dropout_keyed(x, p, ids_t, ops.train_key(seed + 1, step, DEV), site)):
        differ = ((other != 0) != keep).float().mean().item()
        assert abs(differ - 2 * p * (1 - p)) < 0.01
    assert ag.dropout_keyed(x, 0.0, ids_t, key, site) is x


def test_keyed_dropout_rejects_what_it_cannot_run():
    from diff_sal_amd import ops

    key, ids_t = ops.train_key(1, 0, DEV), ops.sample_ids([0, 1], DEV)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.dropout_keyed(torch.ones(2, 7, 9, device=DEV), 0.1, ids_t, key, 0)
    with pytest.raises(ValueError, match="site"):
        ops.dropout_keyed(torch.ones(2, 8, device=DEV), 0.1, ids_t, key, 13)
    with pytest.raises(ValueError, match="one id per sample"):
        ops.dropout_keyed(torch.ones(3, 8, device=DEV), 0.1, ids_t, key, 0)
    with pytest.raises(ValueError, match="key"):
        ops.dropout_keyed(torch.ones(2, 8, device=DEV), 0.1, ids_t, key[:1], 0)


def test_what_a_sample_sees_does_not_depend_on_the_layout():
    """Operator level (in train mode BatchNorm couples the samples of a batch, so no whole-network claim): six ids as one batch of
    6, as 4 + 2, and as six singles in permuted order."""
    from diff_sal_amd import ops

    seed, step, hw = 99, 4, (64, 128)
    ta, tb = _tables()
    ta, tb = ta.to(DEV), tb.to(DEV)
    key = ops.train_key(seed, step, DEV)
    sal = _sal(6, hw, "layout")
    drop_in = [(torch.rand((6, 8, 12, c), generator=torch.Generator().manual_seed(c)) + 0.5).to(DEV) for c in (32, 64, 100)]

    def run(ids, rows, mode="per_sample"):
        ids_t = ops.sample_ids(ids, DEV)
        outs = list(ops.train_prepare(sal[rows].contiguous(), ids_t, key, ta, tb, t_mode=mode))
        outs += [ops.dropout_keyed(d[rows].contiguous(), 0.1, ids_t, key, i) != 0 for i, d in enumerate(drop_in)]
        return outs

    whole = run(IDS6, list(range(6)))
    split = [torch.cat(pair) for pair in zip(run(IDS6[:4], [0, 1, 2, 3]), run(IDS6[4:], [4, 5]))]
    single = [None] * 6
    for i in (4, 0, 5, 2, 1, 3):
        single[i] = run([IDS6[i]], [i])
    single = [torch.cat(parts) for parts in zip(*single)]
    for name, w, s, o in zip(("x0", "x_t", "t", "noise", "mask0", "mask1", "mask2"), whole, split, single):
        assert torch.equal(w, s) and torch.equal(w, o), name
    assert whole[2].tolist() == [_ref_t(seed, step, i) for i in IDS6] and len(set(whole[2].tolist())) > 1
    # batch mode: the draw of the first id of the call, whatever the others are
    for ids, rows in ((IDS6, list(range(6))), (IDS6[4:], [4, 5]), ([IDS6[2]], [2])):
        assert run(ids, rows, "batch")[2].tolist() == [_ref_t(seed, step, ids[0])] * len(ids)


# ---- whole steps on tiny_av ----
def _tiny(B, tag="tn"):
    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    _, feats, audio = orc.synth_inputs(cfg, B, True, tag=tag)
    sal = torch.sigmoid(orc.synth_tensor(tag + ".sal", (B, 1, *cfg.img_size))).to(DEV)
    return cfg, sd, sal, {"feat_list": [f.to(DEV) for f in feats], "audio_feat": audio.to(DEV)}


def test_device_step_is_the_torch_step_fed_the_same_noise():
    """Ties the new path to the verified one: dropout off, a fixed t0; the torch-noise step gets the two noise tensors from
    ops.philox_normal.  Loss and updated parameters bit-equal."""
    from diff_sal_amd import ops
    from diff_sal_amd.train_step import DiffusionTrainStep

    cfg, sd, sal, cond = _tiny(2)
    seed, ids, t0 = 21, [1 << 36, 8], 412
    results = []
    for source in ("device", "torch"):
        net = build(cfg, sd)
        net.dropout_p = 0.0
        ts = DiffusionTrainStep(net, lr=1e-4, grad_clip=1.0, noise_source=source, seed=seed)
        for step in range(2):
            step_ids = [i + step for i in ids]
            if source == "device":
                loss = ts.step(sal, cond, t0=t0, sample_ids=step_ids)
            else:
                shape = tuple(sal.shape[1:])
                z0 = ops.philox_normal(step_ids, seed, ops.train_draw(step, ops.TRAIN_DEQUANT), shape)
                z1 = ops.philox_normal(step_ids, seed, ops.train_draw(step, ops.TRAIN_NOISE), shape)
                loss = ts.step(sal, cond, t0=t0, noise=z1, dequant_noise=z0)
            results.append((source, step, loss.clone()))
        results.append((source, "params", ts.flat.flat_p.clone()))
    half = len(results) // 2
    for (_, what, a), (_, _, b) in zip(results[:half], results[half:]):
        assert torch.equal(a, b), what
    print("losses", [r[2].item() for r in results[:2]])


def _run_steps(make_model, cond_of, sal, n_steps, seed, start=None, first=0):
    """``n_steps`` device-noise steps (dropout 0.1, per-sample timesteps, ids that change every step) on a fresh model; ``start`` =
    (module state_dict, optimizer state_dict) continues a run at step ``first``."""
    from diff_sal_amd.train_step import DiffusionTrainStep

    model = make_model(None if start is None else start[0])
    ts = DiffusionTrainStep(model, lr=1e-4, grad_clip=1.0, noise_source="device", seed=seed, t_mode="per_sample")
    if start is not None:
        ts.load_state_dict(start[1])
        assert ts.step_count == first
    losses = []
    for step in range(first, first + n_steps):
        ids = [(1 << 34) + 1000 * step + 3, 7 + step]
        losses.append(ts.step(sal, cond_of(model), sample_ids=ids).clone())
    assert ts.train_key.tolist() == [seed, ts.step_count] and ts.step_count == first + n_steps
    return model, ts, losses


def _check_determinism_and_resume(make_model, cond_of, sal):
    seed = 31
    _, ts_a, la = _run_steps(make_model, cond_of, sal, 4, seed)
    _, ts_b, lb = _run_steps(make_model, cond_of, sal, 4, seed)
    # the premise: the same four steps twice
    assert torch.equal(ts_a.flat.flat_p, ts_b.flat.flat_p) and all(torch.equal(x, y) for x, y in zip(la, lb))
    assert not torch.equal(la[0], la[1])
    m1, ts1, l1 = _run_steps(make_model, cond_of, sal, 2, seed)
    module_sd = {k: v.detach().cpu().clone() for k, v in m1.state_dict().items()}
    optim_sd = ts1.state_dict()
    assert set(optim_sd) == {"state", "param_groups"}                 # the checkpoint format is what it was
    _, ts2, l2 = _run_steps(make_model, cond_of, sal, 2, seed, start=(module_sd, optim_sd), first=2)
    assert all(torch.equal(x, y) for x, y in zip(l1 + l2, la))
    assert torch.equal(ts2.flat.flat_p, ts_a.flat.flat_p)
    assert torch.equal(ts2.flat.exp_avg, ts_a.flat.exp_avg) and torch.equal(ts2.flat.exp_avg_sq, ts_a.flat.exp_avg_sq)
    # another seed is another run
    _, ts_c, _ = _run_steps(make_model, cond_of, sal, 1, seed + 1)
    _, ts_d, _ = _run_steps(make_model, cond_of, sal, 1, seed)
    assert not torch.equal(ts_c.flat.flat_p, ts_d.flat.flat_p)


def test_training_run_is_deterministic_and_resumes_exactly():
    cfg, sd, sal, cond = _tiny(2)

    def make_model(state):
        return build(cfg, sd if state is None else state)

    _check_determinism_and_resume(make_model, lambda m: cond, sal)


def test_resume_through_video_saliency_model_with_a_torch_encoder(monkeypatch):
    """The dropout key reaches the SalUNet nested in a VideoSaliencyModel: the same resume check, and every dropout launch of
    the steps is the keyed one."""
    from diff_sal_amd import VideoSaliencyModel, ops

    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    H, W = cfg.img_size

    class ToyEncoder(torch.nn.Module):       # clip [B,3,8,H,W] -> 4 feature maps, coarsest first; products only (bit-reproducible)
        def __init__(self):
            super().__init__()
            self.proj = torch.nn.ModuleList([torch.nn.Linear(3, c) for c in cfg.up_channel])

        def forward(self, clip):
            outs = []
            for p, s in zip(self.proj, (32, 16, 8, 4)):
                pooled = torch.nn.functional.adaptive_avg_pool3d(clip, (8, H // s, W // s))
                outs.append(p(pooled.permute(0, 2, 3, 4, 1)).permute(0, 4, 1, 2, 3).contiguous())
            return outs

    def make_model(state):
        torch.manual_seed(0)
        model = VideoSaliencyModel(channel_list=None, visual_net=ToyEncoder(), decoder_net=build(cfg, sd)).to(DEV)
        if state is not None:
            model.load_state_dict(state)
        return model

    g = torch.Generator().manual_seed(5)
    clip = torch.randn((2, 3, 8, H, W), generator=g).to(DEV)
    sal = torch.rand((2, 1, H, W), generator=g).to(DEV)
    calls = {"keyed": 0, "hashed": 0}
    keyed, hashed = ops.dropout_keyed, ops.dropout
    monkeypatch.setattr(ops, "dropout_keyed", lambda *a, **k: calls.__setitem__("keyed", calls["keyed"] + 1) or keyed(*a, **k))
    monkeypatch.setattr(ops, "dropout", lambda *a, **k: calls.__setitem__("hashed", calls["hashed"] + 1) or hashed(*a, **k))
    _check_determinism_and_resume(make_model, lambda m: {"img": clip}, sal)
    assert calls["hashed"] == 0 and calls["keyed"] == 6 * 14           # 3 sites, forward and backward, 14 steps in all
    assert make_model(None).decoder_net._dropout_key is None


def test_training_target_noise():
    """loss = mse_weight / B * sum (pred - noise)^2, recomputed in fp64 from the step's own prediction and noise."""
    from diff_sal_amd.train_step import DiffusionTrainStep

    cfg, sd, sal, cond = _tiny(2)
    net = build(cfg, sd)
    w, ids = 0.7, [12, 1 << 33]
    ts = DiffusionTrainStep(net, lr=1e-4, mse_weight=w, noise_source="device", seed=4, t_mode="per_sample", training_target="noise")
    seen = []
    net.register_forward_hook(lambda mod, args, out: seen.append(out.detach().clone()))
    x0, _, _, noise = ts.prepare_data(sal, sample_ids=ids)            # a pure function of (seed, step, ids): what the step draws
    loss = ts.step(sal, cond, sample_ids=ids).item()
    assert len(seen) == 1
    want = w / 2 * (seen[0].double() - noise.double()).square().sum().item()
    other = w / 2 * (seen[0].double() - x0.double()).square().sum().item()
    print(f"loss {loss:.6f}, fp64 on noise {want:.6f}, on x0 {other:.6f}")
    assert abs(loss - want) <= 1e-6 * abs(want) and abs(loss - other) > 1e-3 * abs(want)
    # the loss_fn face sees the same target
    got = []
    net2 = build(cfg, sd)

    def loss_fn(pred, target):
        got.append(target)
        return (pred - target).square().sum() * 0.5

    ts2 = DiffusionTrainStep(net2, noise_source="device", seed=4, t_mode="per_sample", training_target="noise", loss_fn=loss_fn)
    ts2.step(sal, cond, sample_ids=ids)
    assert torch.equal(got[0], noise)
