"""DiffusionTrainStep(hip_graph=True): a step replayed from a captured HIP graph is the eager step, bit for bit.

Every comparison is ``torch.equal`` against an eager twin: a second trainer built from the same weights and seed with
``hip_graph=False``.  Unless a test says otherwise: ``noise_source="device"``, ``t_mode="per_sample"``, dropout 0.1,
``grad_clip=1.0``, the ``tiny_av`` denoiser at B = 2."""
import os
import socket
import time
import types

import pytest
import torch
import torch.multiprocessing as mp

from oracle import salunet_oracle as orc
from tests._cases import CASES
from tests.test_gpu_salunet import build

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 31
KW = dict(lr=1e-4, grad_clip=1.0, noise_source="device", seed=SEED, t_mode="per_sample")


def _ids(step, B=2):
    return [(1 << 34) + 1000 * step + 3, 7 + step][:B]


def _tiny(B=2, tag="tg"):
    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    _, feats, audio = orc.synth_inputs(cfg, B, True, tag=tag)
    sal = torch.sigmoid(orc.synth_tensor(tag + ".sal", (B, 1, *cfg.img_size))).to(DEV)
    return cfg, sd, sal, {"feat_list": [f.to(DEV) for f in feats], "audio_feat": audio.to(DEV)}


def _trainer(model, graph, **kw):
    from diff_sal_amd.train_step import DiffusionTrainStep

    args = dict(KW)
    args.update(kw)
    return DiffusionTrainStep(model, hip_graph=graph, **args)


def _steps(ts, sal, cond, steps, after=None):
    """-> per step (loss, last_norm, last_losses) as clones; ``after(step)`` runs after each step"""
    out = []
    for step in steps:
        loss = ts.step(sal, cond, sample_ids=_ids(step, sal.shape[0]))
        losses = None if ts.last_losses is None else {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ts.last_losses.items()}
        out.append((loss.clone(), ts.last_norm.clone(), losses))
        if after is not None:
            after(step)
    return out


def _same_steps(got, want):
    assert len(got) == len(want)
    for k, ((la, na, da), (lb, nb, db)) in enumerate(zip(got, want)):
        assert torch.equal(la, lb), f"loss of step {k}: {la.item()} vs {lb.item()}"
        assert torch.equal(na, nb), f"norm of step {k}"
        assert (da is None) == (db is None)
        if da is not None:
            assert set(da) == set(db)
            for key in da:
                if torch.is_tensor(da[key]):
                    assert torch.equal(da[key], db[key]), f"last_losses[{key!r}] of step {k}"
                else:
                    assert da[key] == db[key], key


def _same_state(a, b):
    assert torch.equal(a.flat.flat_p, b.flat.flat_p)
    assert torch.equal(a.flat.exp_avg, b.flat.exp_avg) and torch.equal(a.flat.exp_avg_sq, b.flat.exp_avg_sq)
    bufs_a, bufs_b = dict(a.model.named_buffers()), dict(b.model.named_buffers())
    assert set(bufs_a) == set(bufs_b) and any("num_batches_tracked" in k for k in bufs_a)
    for k in bufs_a:
        assert torch.equal(bufs_a[k], bufs_b[k]), k
    assert a.train_key.tolist() == b.train_key.tolist() and a.step_count == b.step_count


# ---- 1. the optimizer kernel that reads its numbers from memory ----
@pytest.mark.parametrize("store", [0, 1])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_step_args_is_adam_step(step, clip, store):
    """n = 4099 (a vector tail of three); one update and three chained ones; weight decay in one case."""
    from diff_sal_amd import ops

    n, gscale = 4099, 0.5
    wd = 0.01 if (step == 2 and clip) else 0.0
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    max_norm = 1.0 if clip else 0.0
    g = torch.Generator().manual_seed(step)
    p0, m0 = torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g)
    v0 = 0.01 * torch.rand(n, generator=g)
    grads = [(3.0 * torch.randn(n, generator=g)).to(DEV) for _ in range(3)]
    a = [t.to(DEV).clone() for t in (p0, m0, v0)]
    b = [t.to(DEV).clone() for t in (p0, m0, v0)]
    assert ops.adam_args_size() == 36
    block_dev = torch.zeros(64, dtype=torch.uint8, device=DEV)
    for k, grad in enumerate(grads):
        ga, gb = grad.clone(), grad.clone()
        norm = ops.grad_norm(grad, gscale) if clip else None
        ops.adam_step(a[0], ga, a[1], a[2], step=step + k, gscale=gscale, norm=norm, max_norm=max_norm, store_clipped_grad=bool(store), **hp)
        block = ops.adam_args(step=step + k, gscale=gscale, max_norm=max_norm, **hp)
        assert block.dtype == torch.uint8 and block.numel() == 36 and not block.is_cuda and block.is_pinned()
        block_dev[:36].copy_(block, non_blocking=True)
        ops.adam_step_args(b[0], gb, b[1], b[2], block_dev, norm, bool(store))
        for name, x, y in zip("pmvg", a + [ga], b + [gb]):
            assert torch.equal(x, y), f"{name} after {k + 1} update(s)"
        assert torch.equal(ga, grad) == (not store or (not clip and gscale == 1.0))
    assert not torch.equal(a[0], p0.to(DEV))


# ---- 2. the test that fails without the feature ----
def test_graph_steps_are_eager_steps():
    """Six steps, ids that change every step, lr times 0.1 between steps 4 and 5 through MultiStepLR: two eager warm-up steps,
    ONE capture, four replays; losses, norms, parameters, moments, every buffer and the train key equal the twin's."""
    cfg, sd, sal, cond = _tiny()
    runs = {}
    for graph in (False, True):
        ts = _trainer(build(cfg, sd), graph)
        sched = torch.optim.lr_scheduler.MultiStepLR(ts.optimizer, milestones=[4], gamma=0.1)
        lrs = []
        runs[graph] = (ts, _steps(ts, sal, cond, range(6), after=lambda s: (lrs.append(ts.lr), sched.step())), lrs)
    (eager, want, lrs_e), (graphed, got, lrs_g) = runs[False], runs[True]
    assert lrs_e == lrs_g == [1e-4] * 4 + [pytest.approx(1e-5)] * 2
    _same_steps(got, want)
    _same_state(graphed, eager)
    assert graphed.step_count == 6 and graphed.train_key.tolist() == [SEED, 6]
    assert (graphed.graph_captures, graphed.graph_replays) == (1, 4)
    assert (eager.graph_captures, eager.graph_replays) == (0, 0)
    assert not torch.equal(want[4][0], want[5][0])
    # the returned loss is the static tensor: one object for every replay of the signature
    l6 = graphed.step(sal, cond, sample_ids=_ids(6))
    l7 = graphed.step(sal, cond, sample_ids=_ids(7))
    assert l6 is l7 and graphed.graph_replays == 6


# ---- 3. VideoSaliencyModel with the reference's loss dictionary ----
class ToyEncoder(torch.nn.Module):       # clip [B,3,8,H,W] -> 4 feature maps, coarsest first (the pattern of test_gpu_train_noise.py)
    def __init__(self, cfg):
        super().__init__()
        self.hw = cfg.img_size
        self.proj = torch.nn.ModuleList([torch.nn.Linear(3, c) for c in cfg.up_channel])

    def forward(self, clip):
        H, W = self.hw
        outs = []
        for p, s in zip(self.proj, (32, 16, 8, 4)):
            pooled = torch.nn.functional.adaptive_avg_pool3d(clip, (8, H // s, W // s))
            outs.append(p(pooled.permute(0, 2, 3, 4, 1)).permute(0, 4, 1, 2, 3).contiguous())
        return outs


def test_video_saliency_model_with_loss_config():
    from diff_sal_amd import VideoSaliencyModel

    cfg = CASES["tiny_av"][0]
    sd = orc.synth_state_dict(orc.state_dict_template(cfg))
    H, W = cfg.img_size
    lc = types.SimpleNamespace(loss_kl=False, loss_ce=False, loss_mse=True, mse_weight=1.0, loss_cc=True, cc_weight=-0.3,
                               loss_sim=True, sim_weight=-0.2, loss_nss=True, nss_weight=-0.1)
    config = types.SimpleNamespace(loss=lc)
    g = torch.Generator().manual_seed(5)
    clip = torch.randn((2, 3, 8, H, W), generator=g).to(DEV)
    sal = torch.rand((2, 1, H, W), generator=g).to(DEV)
    runs = {}
    for graph in (False, True):
        torch.manual_seed(0)
        model = VideoSaliencyModel(channel_list=None, visual_net=ToyEncoder(cfg), decoder_net=build(cfg, sd)).to(DEV)
        ts = _trainer(model, graph, loss_config=config)
        runs[graph] = (ts, _steps(ts, sal, {"img": clip}, range(4)))
    want, got = runs[False][1], runs[True][1]
    assert set(want[0][2]) == {"total", "main", "cc", "sim", "nss"} and all(float(want[0][2][k]) != 0.0 for k in want[0][2])
    _same_steps(got, want)
    assert torch.equal(runs[True][0].flat.flat_p, runs[False][0].flat.flat_p)
    assert (runs[True][0].graph_captures, runs[True][0].graph_replays) == (1, 2)


# ---- 4. the HIP encoders on their training paths ----
def test_full_audio_visual_model_with_the_hip_encoders():
    """MViT + frozen VGGish + AudioAttnNet + SalUNet at 64 x 128, B = 2: two eager warm-up steps and two replays are four
    eager steps."""
    from diff_sal_amd.diff_model import VideoSaliencyModel
    from tests.test_gpu_encoder_train import rnd
    from tests.test_gpu_encoders import build_audio, build_mvit

    cfg = orc.SalUNetConfig(img_size=(64, 128))
    dsd = orc.synth_state_dict(orc.state_dict_template(cfg))
    B = 2
    data = {"img": rnd("gavt.clip", B, 3, 16, 64, 128).to(DEV), "audio": rnd("gavt.audio", B, 1, 9, 32, 64).to(DEV)}
    sal = torch.sigmoid(rnd("gavt.sal", B, 1, 64, 128)).to(DEV)
    runs = {}
    for graph in (False, True):
        torch.manual_seed(0)            # VideoSaliencyModel draws its own head's initial weights from torch's generator
        enc = build_mvit("small")[0]
        enc.requires_grad_(True)
        vgg, aan = build_audio()[:2]
        model = VideoSaliencyModel(channel_list=None, visual_net=enc, audio_net=vgg, spatiotemp_net=aan, decoder_net=build(cfg, dsd)).to(DEV)
        ts = _trainer(model, graph)
        runs[graph] = (ts, _steps(ts, sal, data, range(4)))
    _same_steps(runs[True][1], runs[False][1])
    assert torch.equal(runs[True][0].flat.flat_p, runs[False][0].flat.flat_p)
    assert (runs[True][0].graph_captures, runs[True][0].graph_replays) == (1, 2)


# ---- 5. checkpoints ----
def test_resume_into_a_fresh_trainer_and_into_a_live_capture():
    """graph_warmup=1, so that two steps already hold a capture.  The checkpoint format is unchanged; a fresh graph trainer that
    loads it, and the capturing trainer itself after loading it back, both go on as the eager run does."""
    cfg, sd, sal, cond = _tiny()
    eager = _trainer(build(cfg, sd), False)
    want = _steps(eager, sal, cond, range(4))
    first = _trainer(build(cfg, sd), True, graph_warmup=1)
    got = _steps(first, sal, cond, range(2))
    assert (first.graph_captures, first.graph_replays) == (1, 1)
    module_sd = {k: v.detach().cpu().clone() for k, v in first.model.state_dict().items()}
    optim_sd = first.state_dict()
    assert set(optim_sd) == {"state", "param_groups"}
    pointers = [t.data_ptr() for t in (first.train_key, first.flat.flat_p, first.flat.exp_avg, first.flat.exp_avg_sq)]
    got += _steps(first, sal, cond, range(2, 4))
    _same_steps(got, want)
    _same_state(first, eager)
    # back to step 2 under the live capture, in place
    first.model.load_state_dict(module_sd)
    first.load_state_dict(optim_sd)
    assert pointers == [t.data_ptr() for t in (first.train_key, first.flat.flat_p, first.flat.exp_avg, first.flat.exp_avg_sq)]
    assert first.step_count == 2 and first.train_key.tolist() == [SEED, 2]
    again = _steps(first, sal, cond, range(2, 4))
    _same_steps(again, want[2:])
    _same_state(first, eager)
    assert (first.graph_captures, first.graph_replays) == (1, 5)
    # a fresh trainer
    fresh = _trainer(build(cfg, module_sd), True, graph_warmup=1)
    fresh.load_state_dict(optim_sd)
    _same_steps(_steps(fresh, sal, cond, range(2, 4)), want[2:])
    _same_state(fresh, eager)
    assert (fresh.graph_captures, fresh.graph_replays) == (1, 1)


# ---- 6. one capture per signature ----
def test_a_capture_per_signature_and_the_old_one_when_it_returns():
    cfg, sd, sal, cond = _tiny()
    one = (sal[:1].contiguous(), {"feat_list": [f[:1].contiguous() for f in cond["feat_list"]], "audio_feat": cond["audio_feat"][:1].contiguous()})
    plan = [(sal, cond)] * 4 + [one] * 3 + [(sal, cond)] * 2
    runs = {}
    for graph in (False, True):
        ts = _trainer(build(cfg, sd), graph)
        out = []
        for step, (s, c) in enumerate(plan):
            out += _steps(ts, s, c, [step])
        runs[graph] = (ts, out)
    _same_steps(runs[True][1], runs[False][1])
    _same_state(runs[True][0], runs[False][0])
    # B = 2: two warm-up steps, capture, 2 + 2 replays;  B = 1: one warm-up step of its own, capture, 2 replays
    assert (runs[True][0].graph_captures, runs[True][0].graph_replays) == (2, 6)


# ---- 7. eval after graph steps ----
def test_eval_forward_sees_the_replayed_updates():
    cfg, sd, sal, cond = _tiny()
    x, _, _ = orc.synth_inputs(cfg, 2, True, tag="tg.eval")
    t = torch.tensor([300, 700], device=DEV)
    preds = {}
    for graph in (False, True):
        net = build(cfg, sd)
        with torch.no_grad():
            first = net(x.to(DEV), t, cond["feat_list"], cond["audio_feat"]).clone()      # fills the eval caches with the initial weights
        ts = _trainer(net, graph, lr=2e-3)          # large steps: stale packed weights would show
        _steps(ts, sal, cond, range(3))
        net.eval()
        with torch.no_grad():
            preds[graph] = net(x.to(DEV), t, cond["feat_list"], cond["audio_feat"]).clone()
        assert not torch.equal(preds[graph], first)
        if graph:
            assert ts.graph_replays == 1
    assert torch.equal(preds[True], preds[False])


# ---- 8. argument rules ----
def test_rules():
    from diff_sal_amd.train_step import DiffusionTrainStep

    cfg, sd, sal, cond = _tiny()
    with pytest.raises(ValueError, match="noise_source='device'"):
        DiffusionTrainStep(build(cfg, sd), hip_graph=True, noise_source="torch")
    with pytest.raises(ValueError, match="noise_source='device'"):
        DiffusionTrainStep(build(cfg, sd), hip_graph=True)
    eager, graphed = _trainer(build(cfg, sd), False), _trainer(build(cfg, sd), True)
    want = _steps(eager, sal, cond, range(3))
    got = _steps(graphed, sal, cond, range(3))
    assert (graphed.graph_captures, graphed.graph_replays) == (1, 1)
    for ts, out in ((eager, want), (graphed, got)):         # a fixed timestep: an eager step on both
        loss = ts.step(sal, cond, t0=412, sample_ids=_ids(3))
        out.append((loss.clone(), ts.last_norm.clone(), None))
    assert (graphed.graph_captures, graphed.graph_replays) == (1, 1)
    want += _steps(eager, sal, cond, [4])
    got += _steps(graphed, sal, cond, [4])
    assert (graphed.graph_captures, graphed.graph_replays) == (1, 2)
    _same_steps(got, want)
    _same_state(graphed, eager)


# ---- 9. two ranks on one GPU ----
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, graph, ret):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, sd, sal, cond = _tiny(tag=f"tg.rank{rank}")
    ts = _trainer(build(cfg, sd), graph, bucket_mb=0.25)
    assert ts.world == 2 and len(ts.flat.buckets) >= 3
    losses = []
    for step in range(4):
        losses.append(ts.step(sal, cond, sample_ids=[_ids(step)[rank], 100 + 2 * step + rank]).item())
    ret[(graph, rank)] = dict(p=ts.flat.flat_p.cpu(), losses=losses, order=list(ts.reducer.launch_order),
                              collectives=list(ts.reducer.collectives), counts=(ts.graph_captures, ts.graph_replays),
                              key=ts.train_key.tolist())
    dist.destroy_process_group()


def _spawn(graph, ret, deadline_s=150.0):
    world = 2
    ctx = mp.start_processes(_worker, args=(world, _free_port(), graph, ret), nprocs=world, join=False, start_method="spawn")
    end = time.monotonic() + deadline_s
    try:
        while not ctx.join(timeout=1.0):
            if time.monotonic() > end:
                raise AssertionError(f"the ranks (hip_graph={graph}) did not finish in {deadline_s:.0f} s")
    finally:
        for proc in ctx.processes:
            if proc.is_alive():
                proc.kill()
        for proc in ctx.processes:
            proc.join(10)


def test_two_ranks_with_the_deferred_exchange():
    """Four steps on two ranks (gloo carries the GPU buffers, as in test_gpu_train_dist.py), eager and graph: same losses and
    parameters on each rank, the collectives of a replayed step in the eager step's order and form."""
    with mp.Manager() as mgr:
        shared = mgr.dict()
        for graph in (False, True):
            _spawn(graph, shared)
        ret = dict(shared)
    for rank in range(2):
        e, g = ret[(False, rank)], ret[(True, rank)]
        assert g["losses"] == e["losses"] and torch.equal(g["p"], e["p"])
        assert g["order"] == e["order"] == list(range(len(e["order"]))) and len(e["order"]) >= 3
        assert g["collectives"] == e["collectives"] and len(e["collectives"]) == len(e["order"])
        assert g["key"] == e["key"] == [SEED, 4]
        assert e["counts"] == (0, 0) and g["counts"] == (1, 2)
    assert torch.equal(ret[(True, 0)]["p"], ret[(True, 1)]["p"])
    assert ret[(True, 0)]["losses"] != ret[(True, 1)]["losses"]
