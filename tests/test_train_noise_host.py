"""Device training noise (include/diffsal.h "training noise") without a GPU: the three C entries are declared and validate their
arguments before any launch, the host mirror of the draw word, and the argument rules of DiffusionTrainStep / SalUNet."""
import os
import re

import pytest
import torch

from diff_sal_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("diffsal_train_prepare", "diffsal_dropout_keyed", "diffsal_train_key_advance")


def test_the_three_entries_are_declared_in_the_header_and_bound():
    text = open(os.path.join(ROOT, "include", "diffsal.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in include/diffsal.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_entries_validate_their_arguments_without_a_gpu():
    """Validation happens before any launch.  16 stands for a (never dereferenced) non-null device pointer."""
    lib = _lib.load()
    E_SHAPE, E_ALIGN, E_ARG = -1, -2, -4

    def prepare(sal=16, ids=16, key=16, ta=16, tb=16, T=1000, dq=0.01, mode=0, tf=0, x0=16, xt=16, t=16, noise=None, B=2, per=64):
        return lib.diffsal_train_prepare(sal, ids, key, ta, tb, T, dq, mode, tf, x0, xt, t, noise, B, per, None)

    for missing in ("sal", "ids", "key", "ta", "tb", "x0", "xt", "t"):
        assert prepare(**{missing: None}) == E_ARG and b"train_prepare: null" in lib.diffsal_last_error(), missing
    assert prepare(B=0) == E_SHAPE and b"shape" in lib.diffsal_last_error()
    assert prepare(per=0) == E_SHAPE
    assert prepare(per=(1 << 34) + 1) == E_SHAPE and b"per" in lib.diffsal_last_error()
    assert prepare(T=0) == E_SHAPE and b"T" in lib.diffsal_last_error()
    assert prepare(T=(1 << 31) + 1) == E_SHAPE
    assert prepare(mode=3) == E_ARG and b"t_mode" in lib.diffsal_last_error()
    assert prepare(mode=2, tf=1000) == E_SHAPE and b"timestep" in lib.diffsal_last_error()
    assert prepare(mode=2, tf=-1) == E_SHAPE

    def drop(x=16, out=16, B=2, per=64, p=0.1, ids=16, key=16, site=0):
        return lib.diffsal_dropout_keyed(x, out, B, per, p, ids, key, site, None)

    for missing in ("x", "out", "ids", "key"):
        assert drop(**{missing: None}) == E_ARG and b"dropout_keyed: null" in lib.diffsal_last_error(), missing
    assert drop(per=62) == E_SHAPE and b"multiple of 4" in lib.diffsal_last_error()
    assert drop(B=0) == E_SHAPE and drop(per=0) == E_SHAPE
    assert drop(p=1.0) == E_SHAPE and drop(p=-0.1) == E_SHAPE and b"p=" in lib.diffsal_last_error()
    assert drop(site=13) == E_ARG and drop(site=-1) == E_ARG and b"site" in lib.diffsal_last_error()
    assert drop(x=20) == E_ALIGN and drop(out=24) == E_ALIGN

    assert lib.diffsal_train_key_advance(None, None) == E_ARG and b"train_key_advance" in lib.diffsal_last_error()


def test_draw_word_layout_and_step_range():
    from diff_sal_amd import ops

    assert ops.train_draw(0, 0) == 0x80000000
    assert ops.train_draw(0, ops.TRAIN_NOISE) == 0x80000001 and ops.train_draw(0, ops.TRAIN_TIMESTEP) == 0x80000002
    assert ops.train_draw(1, ops.TRAIN_DROPOUT0 + 2) == 0x80000015
    assert ops.train_draw(5, 1) == 0x80000000 | (5 << 4) | 1
    top = ops.train_draw((1 << 27) - 1, 15)
    assert top == 0xFFFFFFFF                                        # the last step fills the word: nothing spills
    # bit 31 apart from the sampler's draws 0, 1, 2, ...; the purposes of one step apart from each other and from the next step
    words = {ops.train_draw(s, p) for s in range(3) for p in range(16)}
    assert len(words) == 48 and all(w >> 31 == 1 for w in words)
    assert (ops.TRAIN_DEQUANT, ops.TRAIN_NOISE, ops.TRAIN_TIMESTEP, ops.TRAIN_DROPOUT0) == (0, 1, 2, 3)
    assert ops.TRAIN_DROPOUT0 + ops.TRAIN_DROPOUT_SITES == 16
    with pytest.raises(ValueError, match="2\\^27"):
        ops.train_draw(1 << 27, 0)
    with pytest.raises(ValueError, match="step"):
        ops.train_draw(-1, 0)
    with pytest.raises(ValueError, match="purpose"):
        ops.train_draw(0, 16)
    # the key is checked before anything is uploaded, and lives on the GPU only
    with pytest.raises(ValueError, match="seed"):
        ops.train_key(1 << 64, 0, "cuda")
    with pytest.raises(ValueError, match="2\\^27"):
        ops.train_key(0, 1 << 27, "cuda")
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.train_key(0, 0, "cpu")


def _toy():
    torch.manual_seed(0)
    return torch.nn.Linear(4, 4)


def test_train_step_argument_rules():
    from diff_sal_amd import ops
    from diff_sal_amd.train_step import DiffusionTrainStep

    ts = DiffusionTrainStep(_toy())
    assert (ts.noise_source, ts.seed, ts.t_mode, ts.training_target) == ("torch", 0, "batch", "x0") and ts.train_key is None
    with pytest.raises(ValueError, match="noise_source"):
        DiffusionTrainStep(_toy(), noise_source="philox")
    with pytest.raises(ValueError, match="t_mode"):
        DiffusionTrainStep(_toy(), noise_source="device", t_mode="each")
    with pytest.raises(ValueError, match="training_target"):
        DiffusionTrainStep(_toy(), training_target="v")
    with pytest.raises(ValueError, match="per_sample.*one t0|per_sample.*ONE t0"):
        DiffusionTrainStep(_toy(), t_mode="per_sample")
    with pytest.raises(ValueError, match="seed"):
        DiffusionTrainStep(_toy(), noise_source="device", seed=-1)

    sal = torch.zeros(2, 1, 4, 6)
    dev = DiffusionTrainStep(_toy(), noise_source="device", seed=7, t_mode="per_sample", training_target="noise")
    with pytest.raises(ValueError, match="sample_ids"):
        dev.step(sal, {})
    with pytest.raises(ValueError, match="sample_ids"):
        dev.prepare_data(sal)
    for kw in (dict(noise=torch.zeros_like(sal)), dict(dequant_noise=torch.zeros_like(sal))):
        with pytest.raises(ValueError, match="noise_source='device'"):
            dev.step(sal, {}, sample_ids=[0, 1], **kw)
        with pytest.raises(ValueError, match="noise_source='device'"):
            dev.prepare_data(sal, sample_ids=[0, 1], **kw)
    for bad in ([0, -1], torch.tensor([-3, 2])):
        with pytest.raises(ValueError, match="non-negative"):
            dev.step(sal, {}, sample_ids=bad)
        with pytest.raises(ValueError, match="non-negative"):
            ops.sample_ids(bad, "cuda")
    with pytest.raises(ValueError, match="one id per sample"):
        dev.step(sal, {}, sample_ids=[0, 1, 2])
    # a CPU tensor: no fallback
    with pytest.raises(RuntimeError, match="GPU only"):
        dev.step(sal, {}, sample_ids=[0, 1])
    with pytest.raises(RuntimeError, match="GPU only"):
        dev.prepare_data(sal, sample_ids=[0, 1], t0=3)
    assert dev.step_count == 0
    # sample ids mean nothing to torch's generator: refused, not ignored
    with pytest.raises(ValueError, match="sample_ids"):
        ts.prepare_data(sal, sample_ids=[0, 1])


def test_default_prepare_data_is_the_torch_path(monkeypatch):
    """With the defaults nothing of the new path runs: the two randn_like draws, numpy's t0 and the two axpbypcz calls."""
    from diff_sal_amd import ops
    from diff_sal_amd.train_step import DiffusionTrainStep

    calls = []
    monkeypatch.setattr(ops, "axpbypcz", lambda x, a, y, b: calls.append((a, b)) or x * a + y * b)
    monkeypatch.setattr(ops, "train_prepare", lambda *a, **k: pytest.fail("the device path ran"))
    ts = DiffusionTrainStep(_toy())
    sal = torch.rand(2, 1, 4, 6)
    torch.manual_seed(3)
    x0, x_t, t, noise = ts.prepare_data(sal, t0=10)
    torch.manual_seed(3)
    dq, nz = torch.randn_like(sal), torch.randn_like(sal)
    assert calls == [(1.0, 0.01), (float(ts.sqrt_alphas_hat[10]), float(ts.sqrt_one_minus_alphas_hat[10]))]
    assert torch.equal(noise, nz) and torch.equal(x0, sal + 0.01 * dq) and t.tolist() == [10, 10]


def test_dropout_seed_and_dropout_key_exclude_each_other():
    from diff_sal_amd.sal_unet import SalUNet

    net = SalUNet.__new__(SalUNet)          # the rule is checked before anything of the module is touched
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(ValueError, match="dropout_seed or dropout_key"):
        SalUNet.forward_train(net, x, torch.zeros(1), [], None, dropout_seed=3, dropout_key=(torch.zeros(1), torch.zeros(2)))
    torch.nn.Module.__init__(net)
    with net.dropout_key_scope((torch.zeros(1), torch.zeros(2))):     # the scoped form counts as given
        assert net._dropout_key is not None
        with pytest.raises(ValueError, match="dropout_seed or dropout_key"):
            SalUNet.forward_train(net, x, torch.zeros(1), [], None, dropout_seed=3)
    assert net._dropout_key is None
    with pytest.raises(RuntimeError, match="GPU only"):      # and the existing CPU refusal is what follows
        SalUNet.forward_train(net, x, torch.zeros(1), [], None, dropout_seed=3)
