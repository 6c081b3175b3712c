"""EMA weights in the training step (``DiffusionTrainStep(ema=...)``): the fused kernel against its parts, the swap, the trainer
against ``EMAHelper`` beside a plain trainer, graph replay, ``ema_weights()``, checkpoints, the driver, two ranks.

Every comparison between two device computations is ``torch.equal``: the fused shadow update is the rounding sequence of
``EMAHelper.update``'s ``axpbypcz`` on the parameters Adam has just written.  The one fp64 comparison has a derived bound."""
import os
import time

import pytest
import torch
import torch.multiprocessing as mp

from oracle import salunet_oracle as orc
from tests import _decoder_bwd_ref as R
from tests.test_gpu_salunet import build
from tests.test_gpu_train_graph import _free_port, _ids, _same_state, _same_steps, _steps, _tiny, _trainer

pytestmark = pytest.mark.gpu
DEV = "cuda"

# ---- 1. the kernel against its parts ----
SIZES = [1, 2, 3, 4, 5, 1023, 1024, 1027, 4096 * 256 * 4 + 1024 + 3]
SWITCHES = [(0.0, False, 0), (0.01, True, 1), (0.0, True, 0), (0.01, False, 1)]      # weight decay, clip, store_clipped_grad
MU, STEP, GSCALE, NORM = 0.999, 3, 0.5, 3.7                                          # 3.7 > max_norm = 1: the clip does clip


@pytest.mark.parametrize("switches", SWITCHES, ids=lambda s: "wd{}-clip{}-store{}".format(*s))
@pytest.mark.parametrize("n", SIZES)
def test_fused_kernel_is_adam_then_the_helpers_update(n, switches):
    from diff_sal_amd import ops

    wd, clip, store = switches
    hp = R.ADAM_HP
    kw = dict(step=STEP, lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=wd, gscale=GSCALE,
              max_norm=hp["max_norm"] if clip else 0.0)
    p, g, m, v = R.adam_operands(n, seed=len(SWITCHES) * SIZES.index(n) + SWITCHES.index(switches))
    s0 = p + 0.05 * torch.randn(n, generator=torch.Generator().manual_seed(n % 1000 + 17))
    norm = torch.tensor([NORM], device=DEV) if clip else None

    def state():
        return [t.to(DEV).clone() for t in (p, g, m, v, s0)]

    a, b, c = state(), state(), state()
    ops.adam_step(*a[:4], norm=norm, store_clipped_grad=bool(store), **kw)
    want_s = ops.axpbypcz(a[0], 1.0 - MU, a[4], MU)                      # EMAHelper.update's call, on the new parameters
    ops.adam_ema_step(*b, norm=norm, store_clipped_grad=bool(store), ema_mu=MU, **kw)
    for name, x, y in zip("pgmv", a, b):
        assert torch.equal(x, y), f"{name} differs from adam_step's"
    assert torch.equal(b[4], want_s), "shadow differs from axpbypcz(p_new, 1 - mu, s_old, mu)"
    if n >= 1023:
        assert not torch.equal(b[0], p.to(DEV)) and not torch.equal(b[4], s0.to(DEV))
    assert torch.equal(b[1], g.to(DEV)) == (not store)

    assert ops.adam_ema_args_size() == ops.adam_args_size() + 8 == 44
    block = ops.adam_ema_args(ema_mu=MU, **kw)
    assert block.dtype == torch.uint8 and block.numel() == 44 and not block.is_cuda
    block_dev = torch.zeros(64, dtype=torch.uint8, device=DEV)
    block_dev[:44].copy_(block, non_blocking=True)
    ops.adam_ema_step_args(*c, block_dev, norm, bool(store))
    for name, x, y in zip("pgmvs", b, c):
        assert torch.equal(x, y), f"{name}: adam_ema_step_args differs from adam_ema_step"

    # fp64.  The parameters first, by the restatement's counted bound; then the shadow from the parameters the kernel wrote:
    # two roundings (the product omm * p, the fma), each at most half an ulp = 2^-24 of its result
    coef = R.adam_coef(GSCALE, NORM if clip else None, kw["max_norm"])
    ref = R.adam_step64(p, g, m, v, step=STEP, wd=wd, coef=coef, lr=hp["lr"], beta1=hp["beta1"], beta2=hp["beta2"], eps=hp["eps"])
    R.check_bound(b[0].cpu().double() - p.double(), ref["step"], ref["tol_step"], "step")
    omm, mu = float(R.f32(1.0 - MU)), float(R.f32(MU))
    p_new = b[0].cpu().double()
    s64 = mu * s0.double() + omm * p_new
    R.check_bound(b[4], s64, 2.0 ** -23 * ((omm * p_new).abs() + s64.abs()), "shadow against fp64")


# ---- 2. the swap ----
SPECIAL = [0x7FC00001, 0x7F800123, 0xFFC0BEEF, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF]


def _bits(n, seed, phase):
    """int32 patterns: every third element from ``phase`` on is a special value (NaNs with payloads, the two zeros, the two
    infinities, denormals) in turn, the rest are random words (any bit pattern, NaNs included)"""
    gen = torch.Generator().manual_seed(seed)
    words = torch.randint(-(1 << 31), 1 << 31, (n,), generator=gen, dtype=torch.int64)
    special = torch.tensor([x - (1 << 32) if x >= 1 << 31 else x for x in SPECIAL], dtype=torch.int64)
    idx = torch.arange(n)
    words = torch.where(idx % 3 == phase, special[(idx // 3) % len(SPECIAL)], words)
    return words.to(torch.int32)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1027, SIZES[-1]])
def test_swap_moves_bits_and_is_its_own_inverse(n):
    from diff_sal_amd import ops

    pb, sb = _bits(n, 1, 0).to(DEV), _bits(n, 2, 1).to(DEV)
    assert not torch.equal(pb, sb)
    p, s = pb.clone().view(torch.float32), sb.clone().view(torch.float32)
    ptrs = (p.data_ptr(), s.data_ptr())
    ops.ema_swap(p, s)
    assert torch.equal(p.view(torch.int32), sb) and torch.equal(s.view(torch.int32), pb)
    ops.ema_swap(p, s)
    assert torch.equal(p.view(torch.int32), pb) and torch.equal(s.view(torch.int32), sb)
    assert ptrs == (p.data_ptr(), s.data_ptr())
    with pytest.raises(RuntimeError, match="same number"):
        ops.ema_swap(p, torch.zeros(n + 1, device=DEV))


# ---- 3. the trainer, eager, against a plain trainer with EMAHelper beside it ----
def _shadow_is(trainer, helper_shadow):
    got = trainer.ema_state_dict()["shadow"]
    assert list(got) == list(helper_shadow) and len(got) > 10
    for name in got:
        assert torch.equal(got[name], helper_shadow[name]), name


@pytest.mark.parametrize("warmup", [False, True])
def test_eager_trainer_is_the_plain_trainer_with_the_helper(warmup):
    from diff_sal_amd.ema import EMAHelper
    from diff_sal_amd.train_step import ema_rate_at

    cfg, sd, sal, cond = _tiny()
    a = _trainer(build(cfg, sd), False, ema=0.9, ema_warmup=warmup)
    b = _trainer(build(cfg, sd), False)
    helper = EMAHelper(mu=0.9)
    helper.register(b.model)
    _shadow_is(a, helper.shadow)

    def update(k):
        helper.mu = ema_rate_at(0.9, k, warmup)
        helper.update(b.model)

    got, want = _steps(a, sal, cond, range(4)), _steps(b, sal, cond, range(4), after=update)
    _same_steps(got, want)
    _same_state(a, b)
    _shadow_is(a, helper.shadow)
    assert a.ema_updates == 4 and helper.mu == (4.0 / 13.0 if warmup else 0.9)
    assert not torch.equal(a.flat.shadow, a.flat.flat_p)
    live = torch.zeros(a.flat.numel, dtype=torch.bool, device=DEV)
    for p, o in zip(a.flat.params, a.flat.offsets):
        live[o:o + p.numel()] = True
    assert not a.flat.shadow[~live].any()                                 # the padding stays zero
    assert set(a.state_dict()) == {"state", "param_groups"}               # torch.optim.Adam's format, unchanged


# ---- 4. the trainer, graph ----
def test_graph_steps_with_a_rate_that_moves_every_step():
    """warm-up: the rate is (1 + k) / (10 + k) < 0.999 at every one of the six steps, so a rate frozen into the capture shows"""
    cfg, sd, sal, cond = _tiny()
    runs = {}
    for graph in (False, True):
        ts = _trainer(build(cfg, sd), graph, ema=0.999, ema_warmup=True)
        sched = torch.optim.lr_scheduler.MultiStepLR(ts.optimizer, milestones=[4], gamma=0.1)
        runs[graph] = (ts, _steps(ts, sal, cond, range(6), after=lambda s: sched.step()))
    (eager, want), (graphed, got) = runs[False], runs[True]
    _same_steps(got, want)
    _same_state(graphed, eager)
    assert torch.equal(graphed.flat.shadow, eager.flat.shadow) and not torch.equal(eager.flat.shadow, eager.flat.flat_p)
    assert (graphed.graph_captures, graphed.graph_replays) == (1, 4) and graphed.ema_updates == eager.ema_updates == 6


# ---- 5. ema_weights() ----
def _eval(net, cfg, cond):
    x, _, _ = orc.synth_inputs(cfg, 2, True, tag="ema.eval")
    net.eval()
    with torch.no_grad():
        return net(x.to(DEV), torch.tensor([300, 700], device=DEV), cond["feat_list"], cond["audio_feat"]).clone()


def test_ema_weights_holds_the_average_and_gives_the_weights_back():
    from diff_sal_amd.ema import EMAHelper

    cfg, sd, sal, cond = _tiny()
    ts = _trainer(build(cfg, sd), False, ema=0.9, lr=2e-3)
    _steps(ts, sal, cond, range(3))
    raw = _eval(ts.model, cfg, cond)
    before, shadow_before = ts.flat.flat_p.clone(), ts.flat.shadow.clone()
    other = build(cfg, {k: v.detach().cpu().clone() for k, v in ts.model.state_dict().items()})      # buffers included
    helper = EMAHelper()
    helper.load_state_dict(ts.ema_state_dict()["shadow"])
    helper.ema(other)
    want = _eval(other, cfg, cond)
    assert not torch.equal(want, raw)
    ptr = ts.flat.flat_p.data_ptr()
    with ts.ema_weights() as inside:
        assert inside is ts and ts.flat.flat_p.data_ptr() == ptr
        assert torch.equal(ts.flat.flat_p, shadow_before) and torch.equal(ts.flat.shadow, before)
        assert torch.equal(_eval(ts.model, cfg, cond), want)
        sd_in = ts.ema_state_dict()["shadow"]                               # still the average
        assert all(torch.equal(sd_in[k], helper.shadow[k]) for k in sd_in)
        with pytest.raises(RuntimeError, match="ema_weights"):
            ts.step(sal, cond, sample_ids=_ids(3))
        with pytest.raises(RuntimeError, match="ema_weights"):
            ts.optimizer_step()
        with pytest.raises(RuntimeError, match="ema_weights"):
            with ts.ema_weights():
                pass
    assert torch.equal(ts.flat.flat_p, before) and torch.equal(ts.flat.shadow, shadow_before)
    assert torch.equal(_eval(ts.model, cfg, cond), raw)
    with pytest.raises(ZeroDivisionError):                                  # an exception inside still gives the weights back
        with ts.ema_weights():
            1 / 0
    assert torch.equal(ts.flat.flat_p, before) and ts.step_count == 3
    ts.step(sal, cond, sample_ids=_ids(3))


def test_ema_weights_under_a_live_capture():
    cfg, sd, sal, cond = _tiny()
    runs = {}
    for graph in (False, True):
        ts = _trainer(build(cfg, sd), graph, graph_warmup=1, ema=0.9, ema_warmup=True)
        out = _steps(ts, sal, cond, range(2))
        with ts.ema_weights():
            mid = _eval(ts.model, cfg, cond)
        out += _steps(ts, sal, cond, range(2, 4))
        runs[graph] = (ts, out, mid)
    _same_steps(runs[True][1], runs[False][1])
    _same_state(runs[True][0], runs[False][0])
    assert torch.equal(runs[True][2], runs[False][2]) and torch.equal(runs[True][0].flat.shadow, runs[False][0].flat.shadow)
    assert (runs[True][0].graph_captures, runs[True][0].graph_replays) == (1, 3)


# ---- 6. resume at trainer level ----
def test_resume_into_a_fresh_trainer():
    cfg, sd, sal, cond = _tiny()
    kw = dict(ema=0.95, ema_warmup=True)
    whole = _trainer(build(cfg, sd), False, **kw)
    want = _steps(whole, sal, cond, range(6))
    first = _trainer(build(cfg, sd), False, **kw)
    _steps(first, sal, cond, range(3))
    module_sd = {k: v.detach().cpu().clone() for k, v in first.model.state_dict().items()}
    optim_sd, ema_sd = first.state_dict(), first.ema_state_dict()
    assert (ema_sd["updates"], ema_sd["mu"], ema_sd["warmup"]) == (3, 0.95, True)
    fresh = _trainer(build(cfg, module_sd), False, **kw)
    fresh.load_state_dict(optim_sd)
    fresh.load_ema_state_dict(ema_sd)
    assert torch.equal(fresh.flat.shadow, first.flat.shadow) and fresh.ema_updates == 3
    _same_steps(_steps(fresh, sal, cond, range(3, 6)), want[3:])
    _same_state(fresh, whole)
    assert torch.equal(fresh.flat.shadow, whole.flat.shadow) and fresh.ema_updates == whole.ema_updates == 6
    name = next(iter(ema_sd["shadow"]))
    keep = fresh.flat.shadow.clone()
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):
        fresh.load_ema_state_dict({"shadow": {k: v for k, v in ema_sd["shadow"].items() if k != name}})
    with pytest.raises(ValueError, match=name.replace(".", r"\.") + ".*shape"):
        fresh.load_ema_state_dict({"shadow": dict(ema_sd["shadow"], **{name: torch.zeros(3, 1, 1, 7)})})
    assert torch.equal(fresh.flat.shadow, keep) and fresh.ema_updates == 6


# ---- 7. the driver ----
SIZE = (64, 128)
UCF3 = ["Act-001", "Act-002", "Act-003"]


@pytest.fixture(scope="module")
def ucf(tmp_path_factory):
    from tests.test_gpu_train import write_ucf_tree

    return write_ucf_tree(str(tmp_path_factory.mktemp("ucf_ema")))


def _make(ema=0.9, lr=1e-3, **kw):
    """tests/test_gpu_train.py's model, and a trainer like its own with the EMA keywords"""
    from diff_sal_amd.train_step import DiffusionTrainStep
    from tests.test_gpu_train import make

    model, _ = make()
    return model, DiffusionTrainStep(model, lr=lr, noise_source="device", seed=5, ema=ema, **kw)


def _log(path):
    return open(path).read()


def test_driver_checkpoints_and_resumes_the_average(ucf, tmp_path):
    from diff_sal_amd import train
    from tests.test_gpu_train import same_state

    kw = dict(size=SIZE, seed=3, videos=UCF3, len_snippet=16, steps_per_load=2)
    whole_dir, cut_dir = str(tmp_path / "whole"), str(tmp_path / "cut")
    model, whole = _make(ema_warmup=True)
    train.fit_directory(model, whole, "ucf", ucf, whole_dir, 2, 2, **kw)
    assert whole.ema_updates == 6 and not torch.equal(whole.flat.shadow, whole.flat.flat_p)
    ck = torch.load(os.path.join(whole_dir, "ckpt_1.pth"), map_location="cpu")
    assert list(ck) == ["state_dict", "optim_dict", "epoch", "step", "ema_dict"]
    assert set(ck["ema_dict"]) == {"shadow", "updates", "mu", "warmup"} and ck["ema_dict"]["updates"] == 3
    model1, first = _make(ema_warmup=True)
    train.fit_directory(model1, first, "ucf", ucf, cut_dir, 2, 2, stop_epoch=1, **kw)
    model2, second = _make(ema_warmup=True)
    report = train.fit_directory(model2, second, "ucf", ucf, cut_dir, 2, 2, resume=os.path.join(cut_dir, "ckpt_1.pth"), **kw)
    assert report.epochs == [2] and second.ema_updates == 6
    assert same_state(whole, second) and torch.equal(whole.flat.shadow, second.flat.shadow)
    head = "\t".join(train.TRAIN_HEADER)
    assert _log(os.path.join(cut_dir, "train.log")).replace("\r", "").replace(head + "\n", "") == \
        _log(os.path.join(whole_dir, "train.log")).replace("\r", "").replace(head + "\n", "")
    a = torch.load(os.path.join(whole_dir, "ckpt_2.pth"), map_location="cpu")["ema_dict"]
    b = torch.load(os.path.join(cut_dir, "ckpt_2.pth"), map_location="cpu")["ema_dict"]
    assert a["updates"] == b["updates"] == 6 and all(torch.equal(a["shadow"][k], b["shadow"][k]) for k in a["shadow"])
    # a checkpoint without ema_dict: the shadow restarts from the loaded weights, no update done
    bare = {k: v for k, v in ck.items() if k != "ema_dict"}
    path = str(tmp_path / "bare.pth")
    torch.save(bare, path)
    assert train.resume_from(path, model2, second) == (1, 3)
    assert second.ema_updates == 0 and torch.equal(second.flat.shadow, second.flat.flat_p)
    assert torch.equal(second.flat.flat_p, first.flat.flat_p) and second.step_count == 3
    with pytest.raises(ValueError, match="ema_dict"):
        train.load_ema_weights(path, model2)


def test_driver_validates_the_average(ucf, tmp_path):
    from diff_sal_amd import predict, train
    from diff_sal_amd.sampling import DiffusionSampler
    from tests.test_gpu_train import LOSS_CFG, make

    def sampler_for(model):
        return DiffusionSampler(model, sample_type="ddim", timesteps=1, noise_source="device", seed=11)

    def fit(name, ema, **more):
        model, trainer = _make(ema=ema, lr=1e-2)      # one large step: the average and the weights validate differently
        out = str(tmp_path / name)
        report = train.fit_directory(model, trainer, "ucf", ucf, out, 1, 2, size=SIZE, seed=3, videos=UCF3[:1], len_snippet=16,
                                     sampler=sampler_for(model), loss_config=LOSS_CFG, val_batch=2, **more)
        return out, report, trainer

    out_a, rep_a, tr_a = fit("a", 0.9)
    out_b, rep_b, _ = fit("b", 0.9, ema_validation=False)
    out_c, rep_c, tr_c = fit("c", None)
    assert _log(os.path.join(out_a, "train.log")) == _log(os.path.join(out_c, "train.log"))
    assert torch.equal(tr_a.flat.flat_p, tr_c.flat.flat_p)
    assert rep_b.val_rows == rep_c.val_rows and _log(os.path.join(out_b, "val.log")) == _log(os.path.join(out_c, "val.log"))
    assert rep_a.val_rows != rep_c.val_rows
    model, _ = make()
    ema_dict = train.load_ema_weights(os.path.join(out_a, "ckpt_1.pth"), model)
    assert ema_dict["updates"] == 1
    for name, p in model.named_parameters():
        if name in ema_dict["shadow"]:
            assert torch.equal(p.detach().cpu(), ema_dict["shadow"][name]), name
    after = predict.predict_directory(model, sampler_for(model), "ucf", ucf, None, batch=2, size=SIZE, losses=True, loss_config=LOSS_CFG,
                                      len_snippet=16, write=False)
    want = train.val_row(1, 1, after.losses)
    assert rep_a.val_rows == [want]
    log = [line.split("\t") for line in _log(os.path.join(out_a, "val.log")).replace("\r", "").splitlines()]
    assert log[1] == [str(want[k]) for k in train.VAL_HEADER]


# ---- 8. two ranks on one GPU ----
def _worker(rank, world, port, graph, ret):
    os.environ.update(RANK=str(rank), LOCAL_RANK="0", WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, sd, sal, cond = _tiny(tag=f"ema.rank{rank}")
    ts = _trainer(build(cfg, sd), graph, bucket_mb=0.25, ema=0.9, ema_warmup=True)
    assert ts.world == 2
    for step in range(3):
        ts.step(sal, cond, sample_ids=[_ids(step)[rank], 100 + 2 * step + rank])
    ret[(graph, rank)] = dict(shadow=ts.flat.shadow.cpu(), p=ts.flat.flat_p.cpu(), updates=ts.ema_updates,
                              counts=(ts.graph_captures, ts.graph_replays))
    dist.destroy_process_group()


def _spawn(graph, ret, deadline_s=150.0):
    """tests/test_gpu_train_graph.py's launcher around this file's worker: two fresh child processes and a deadline"""
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


def test_two_ranks_hold_the_same_shadow():
    with mp.Manager() as mgr:
        shared = mgr.dict()
        for graph in (False, True):
            _spawn(graph, shared)
        ret = dict(shared)
    for graph in (False, True):
        r0, r1 = ret[(graph, 0)], ret[(graph, 1)]
        assert torch.equal(r0["shadow"], r1["shadow"]) and torch.equal(r0["p"], r1["p"])
        assert not torch.equal(r0["shadow"], r0["p"]) and r0["updates"] == r1["updates"] == 3
        assert r0["counts"] == ((1, 1) if graph else (0, 0))
    assert torch.equal(ret[(True, 0)]["shadow"], ret[(False, 0)]["shadow"])
