"""No kernel reads or writes outside its buffers: the case tables of the value tests once more, between guard bands.

Every case body here is the one its value test calls (tests/test_gpu_exact_products.py, test_gpu_instantiations.py,
test_gpu_decoder_bwd.py, test_gpu_encoder_nodes.py, test_gpu_value_range.py): the same operands, the same reference, the same
comparison and bound.  What differs is where the memory comes from.  Inside ``guarded()`` (tests/_guard.py, proved on the CPU by
tests/test_guard_host.py) every torch.empty / zeros / full / ones / *_like of diff_sal_amd/ops.py and autograd_ops.py -- each output
and each workspace -- lies between two bands of 0xFF bytes, and the bodies upload their inputs through ``put``, which surrounds them
with the same bytes (NaN in every floating type).  So a store past a ragged last tile, a workspace a tile short of what its
``*_ws_bytes`` says, or a halo load in front of the image changes a band, or brings a NaN into a result that is compared.

On top of its body's own assertions every case asserts
  (a) ``check()``: both bands of every allocation are untouched;
  (b) every tensor a wrapper of ``ops`` returned lies in a guarded buffer (or is one of the TORCH_COPIES below);
  (c) no CUDA tensor was allocated past the shim through one of the six constructors;
  (d) where the library's ``*_ws_bytes`` / ``*_chunks`` / ``*_blocks`` helper answered non-zero inside a wrapper, that wrapper
      allocated at least one guarded buffer more than it returned.
(b) to (d) keep a case from passing because a wrapper no longer allocates through the shimmed constructors.  They are observed,
not plumbed per entry point: the fixture wraps every public function of ``ops`` and the library binding's helper functions.
"""
import functools
import inspect
import re

import pytest
import torch

from tests import _exact_ref as E
from tests import _guard as G
from tests import _decoder_bwd_ref as DR
from tests import _instantiation_cases as ic
from tests import _train_nodes_ref as TR
from tests import test_gpu_decoder_bwd as DB
from tests import test_gpu_encoder_nodes as EN
from tests import test_gpu_exact_products as XP
from tests import test_gpu_instantiations as IN
from tests import test_gpu_value_range as VR

pytestmark = pytest.mark.gpu
DEV = "cuda"

HELPER = re.compile(r"(_ws_bytes|workspace_bytes|_chunks|_blocks)$")
# (wrapper, position in what it returns): torch's own repacking (.t().contiguous(), torch.cat) of a guarded buffer that a nested
# wrapper returned and that was audited there; no kernel writes these copies
TORCH_COPIES = {("attention_bwd", 1), ("attention_bwd", 2), ("conv_in_bwd", 0)}


def tensors_of(out):
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in tensors_of(o)]
    return []


class Audit:
    """What the wrappers of ``ops`` returned and allocated, and what the library's workspace helpers answered meanwhile."""

    def __init__(self, guard, real_lib):
        self.g, self.real = guard, real_lib
        self.put = guard.put
        self.calls, self.helpers, self.ws_calls = 0, [], 0

    def __getattr__(self, name):                 # the binding's stand-in: _lib.load() returns this object
        fn = getattr(self.real, name)
        if not HELPER.search(name):
            return fn

        def recorded(*args):
            r = fn(*args)
            if r:
                self.helpers.append((name, r))
            return r
        return recorded

    def wrap(self, name, fn):
        @functools.wraps(fn)
        def audited(*args, **kwargs):
            first_buffer, first_helper = len(self.g.buffers), len(self.helpers)
            out = fn(*args, **kwargs)
            if inspect.isgenerator(out) or not tensors_of(out):
                return out
            self.calls += 1
            mine = set()
            for i, t in enumerate(tensors_of(out)):
                if t.device.type != DEV:
                    continue
                assert self.g.owns(t) or (name, i) in TORCH_COPIES, f"(b) ops.{name}: returned tensor {i} {tuple(t.shape)} is in no guarded buffer"
                b = self.g._ptrs.get(t.untyped_storage().data_ptr())
                if b is not None and b.order >= first_buffer:
                    mine.add(b.order)
            asked = self.helpers[first_helper:]
            if asked:
                self.ws_calls += 1
                made = len(self.g.buffers) - first_buffer
                assert made > len(mine), (f"(d) ops.{name}: {asked} is non-zero, but the wrapper made {made} guarded allocations "
                                          f"for the {len(mine)} it returned: its workspace is not guarded")
            return out
        return audited

    def finish(self, ws=None):
        """(a), (c) and that the case went through audited wrappers at all; ``ws``: the case must (True) have met a non-zero helper."""
        torch.cuda.synchronize()
        self.g.check()
        assert not self.g.unguarded_device, "(c) CUDA tensors allocated past the shim:\n  " + "\n  ".join(self.g.unguarded_device)
        assert self.calls > 0 and self.g.guarded > 0 and self.g.puts > 0, (self.calls, self.g.guarded, self.g.puts)
        if ws:
            assert self.ws_calls > 0, "no workspace helper answered non-zero: the case does not reach a guarded workspace"
        print(f"[guard] {self.g.guarded} guarded allocations + {self.g.puts} inputs, {self.g.bytes / 2 ** 20:.1f} MiB, {self.calls} audited "
              f"calls, {self.ws_calls} with a workspace, {self.g.unguarded} unguarded (CPU)")


@pytest.fixture
def guard(monkeypatch):
    from diff_sal_amd import _lib, ops

    assert torch.cuda.is_available()
    real = _lib.load()
    with G.guarded() as g:
        audit = Audit(g, real)
        monkeypatch.setattr(_lib, "_LIB", audit)
        for name, fn in list(vars(ops).items()):
            if inspect.isfunction(fn) and fn.__module__ == ops.__name__ and not name.startswith("_"):
                monkeypatch.setattr(ops, name, audit.wrap(name, fn))
        try:
            yield audit
        finally:
            monkeypatch.undo()


@pytest.fixture(scope="module")
def ops():
    from diff_sal_amd import ops as o

    return o


@pytest.fixture(scope="module")
def dlib():
    from diff_sal_amd import _lib, autograd_ops, ops

    return ops, autograd_ops, _lib


@pytest.fixture(scope="module")
def elib():
    from diff_sal_amd import encoder_autograd, ops

    return ops, encoder_autograd


@pytest.fixture(scope="module")
def agops():
    from diff_sal_amd import autograd_ops

    return autograd_ops


# ---- the detector on the device ----------------------------------------------------------------------------------------------------
def test_a_byte_behind_a_payload_is_seen_and_one_inside_is_not():
    """Both writes are torch indexing writes into the raw uint8 buffer of an allocation this test owns."""
    with pytest.raises(G.GuardError, match=r"allocation #1 \(torch\.empty\) \(5, 3\) torch\.float32 .*back guard changed, 1 bytes, offsets 0 \.\. 0 "):
        with G.guarded() as g:
            torch.zeros(7, device=DEV)
            t = torch.empty((5, 3), device=DEV)
            assert g.owns(t) and t.is_cuda and t.data_ptr() % 256 == 0 and bool(torch.isnan(t).all())
            b = g._ptrs[t.untyped_storage().data_ptr()]
            b.raw[b.start + b.nbytes - 1] = 0            # the payload's last byte
            b.raw[b.start] = 0                           # and its first
            g.check()
            assert g.unguarded_device == [] and g.guarded == 2
            b.raw[b.start + b.nbytes] = 0                # one byte behind
    with pytest.raises(G.GuardError, match=r"front guard changed, 1 bytes, offsets -1 \.\. -1 "):
        with G.guarded() as g:
            t = g.put(torch.arange(6.0))
            b = g._ptrs[t.untyped_storage().data_ptr()]
            b.raw[b.start - 1] = 0x7F


# ---- A. matrix and convolution kernels: bit-equal to fp64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", XP.ROUTES, ids=[r.id for r in XP.ROUTES])
def test_forward_route(guard, ops, tuning, route):
    XP.case_forward_route_equals_fp64(ops, tuning, route, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("case", E.PAIR_CASES, ids=[c[0] for c in E.PAIR_CASES])
def test_linear_pair(guard, ops, tuning, case):
    XP.case_linear_pair_equals_fp64(ops, tuning, case, up=guard.put)
    guard.finish()


def test_linear_group(guard, ops):
    XP.case_linear_group_equals_fp64(ops, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("dname,tile", E.F32OUT_CASES, ids=[f"{d}-tile{t}" for d, t in E.F32OUT_CASES])
def test_linear_fp32_out_of_16bit_operands(guard, ops, tuning, dname, tile):
    XP.case_linear_fp32_out_of_16bit_operands_is_not_rounded(ops, tuning, dname, tile, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("split", [False, True], ids=["split-in-kernel", "split_weight"])
def test_bf16x3(guard, ops, split):
    XP.case_bf16x3_precision_is_exact_on_small_integers(ops, split, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("form", [1, 3])
@pytest.mark.parametrize("i", range(len(E.TAPSUM_CASES)), ids=[str(c) for c in E.TAPSUM_CASES])
def test_tapsum(guard, ops, tuning, i, form):
    XP.case_tapsum_of_tap_weight_products_equals_fp64(ops, tuning, i, form, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("ring_only", [False, True], ids=["direct", "ring_only"])
@pytest.mark.parametrize("i", range(len(E.UP2_CASES)), ids=[str(c) for c in E.UP2_CASES])
def test_up2_conv3x3_d2(guard, ops, tuning, i, ring_only):
    XP.case_up2_conv3x3_d2_equals_fp64(ops, tuning, i, ring_only, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("case", E.WINO_CASES, ids=str)
def test_winograd_f4x4(guard, ops, case):
    XP.case_winograd_f4x4_is_exact_on_an_integer_transform(ops, case, up=guard.put)
    guard.finish(ws=True)


@pytest.mark.parametrize("cfg,dma", XP.WGRAD_ROUTES, ids=[f"cfg{c}-dma{d}" for c, d in XP.WGRAD_ROUTES])
@pytest.mark.parametrize("i", range(len(E.WGRAD_SHAPES)), ids=[str(s) for s in E.WGRAD_SHAPES])
def test_plain_wgrad(guard, ops, tuning, i, cfg, dma):
    XP.case_plain_wgrad_equals_fp64(ops, tuning, i, cfg, dma, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("cfg", E.WGRAD_CFGS)
def test_conv3x3_wgrad(guard, ops, tuning, cfg):
    XP.case_conv3x3_wgrad_equals_fp64(ops, tuning, cfg, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("case", E.SEGMENTED_CASES, ids=str)
def test_wgrad_segmented(guard, ops, case):
    XP.case_wgrad_segmented_equals_fp64(ops, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("case", E.COLSUM_CASES, ids=str)
def test_colsum(guard, ops, case):
    XP.case_colsum_equals_fp64(ops, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("case", E.BACKWARD_CASES, ids=str)
def test_conv_backward(guard, ops, case):
    XP.case_conv_backward_equals_fp64_autograd(ops, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("dma", [0, 1])
def test_linear_backward_with_residual(guard, ops, tuning, dma):
    XP.case_linear_backward_with_residual_equals_fp64_autograd(ops, tuning, dma, up=guard.put)
    guard.finish()


# ---- B. row, attention and pooling instantiations ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ic.ATTN_FWD_CASES, ids=ic.attention_id)
def test_attention_forward_fp32(guard, ops, case):
    IN.run_attention_forward(ops, case, "fp32", "guarded attention fwd fp32", up=guard.put)
    guard.finish()


@pytest.mark.parametrize("generic", [True, False], ids=["generic", "planned"])
@pytest.mark.parametrize("dname", list(IN.DTYPES))
@pytest.mark.parametrize("case", ic.ATTN_FWD_CASES, ids=ic.attention_id)
def test_attention_forward_16bit(guard, ops, tuning, case, dname, generic):
    if generic:
        tuning.set("DIFFSAL_NO_STREAM16", 1)
    IN.run_attention_forward(ops, case, dname, f"guarded attention fwd {dname} {'generic' if generic else 'planned'}", up=guard.put)
    guard.finish()


@pytest.mark.parametrize("case", ic.ATTN_BWD_CASES, ids=ic.attention_id)
def test_attention_backward(guard, ops, case):
    IN.case_attention_backward(ops, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_layernorm_fp32(guard, ops, C):
    IN.run_layernorm(ops, C, "fp32", "guarded layernorm fp32", up=guard.put)
    guard.finish()


@pytest.mark.parametrize("generic", [True, False], ids=["generic", "planned"])
@pytest.mark.parametrize("dname", list(IN.DTYPES))
@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_layernorm_16bit(guard, ops, tuning, C, dname, generic):
    if generic:
        tuning.set("DIFFSAL_NO_STREAM16", 1)
    IN.run_layernorm(ops, C, dname, f"guarded layernorm {dname} {'generic' if generic else 'planned'}", up=guard.put)
    guard.finish()


@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_layernorm_multi(guard, ops, C):
    IN.case_layernorm_multi(ops, C, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_layernorm_backward(guard, ops, C):
    """With and without ``add``, at both row counts of the width."""
    for M in ic.row_counts(C):
        IN.run_layernorm_bwd(ops, C, M, up=guard.put)
    guard.finish(ws=True)


@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_layernorm_backward_multi(guard, ops, C):
    IN.case_layernorm_backward_multi(ops, C, up=guard.put)
    guard.finish(ws=True)


@pytest.mark.parametrize("W", ic.DWCONV_WS)
@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_dwconv3_ln(guard, ops, C, W):
    IN.case_dwconv3_ln(ops, C, W, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_dwpool_ln_kv(guard, ops, C):
    IN.case_dwpool_ln_kv(ops, C, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("W", ic.DWCONV_WS)
@pytest.mark.parametrize("C", ic.ROW_WIDTHS)
def test_qkv_prep(guard, ops, C, W):
    IN.case_qkv_prep_equals_the_two_entries(ops, C, W, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("stride", ic.POOL_STRIDES, ids=IN.pool_id)
@pytest.mark.parametrize("D", ic.POOL_DS, ids=IN.pool_id)
def test_pool3d_ln(guard, ops, D, stride):
    IN.case_pool3d_ln(ops, D, stride, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("stride", ic.POOL_STRIDES, ids=IN.pool_id)
@pytest.mark.parametrize("D", ic.POOL_DS, ids=IN.pool_id)
def test_pool3d_backward(guard, ops, D, stride):
    """dx goes through the strides of one slice of a guarded [B, N, 3, heads, D] buffer: its neighbours and both bands stay NaN."""
    IN.case_pool3d_backward(ops, D, stride, up=guard.put)
    guard.finish(ws=True)


@pytest.mark.parametrize("C,M", ic.LN_PAST_CAP)
def test_layernorm_past_the_grid_cap(guard, ops, C, M):
    IN.case_layernorm_past_the_grid_cap(ops, C, M, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("C,M", ic.LN_BWD_PAST_CAP)
def test_layernorm_backward_past_the_grid_cap(guard, ops, C, M):
    IN.run_layernorm_bwd(ops, C, M, up=guard.put)
    guard.finish(ws=True)


def test_dwconv3_ln_strip_kernel_past_the_grid_cap(guard, ops):
    IN.case_dwconv3_ln_strip_kernel_past_the_grid_cap(ops, up=guard.put)
    guard.finish()


# ---- C. decoder and encoder training kernels, the norm chain ------------------------------------------------------------------------
@pytest.mark.parametrize("case", DR.RESIZE_EXACT, ids=DR.case_id)
def test_resize_adjoint_exact_routes(guard, dlib, case):
    """The routes the raw binding selects take their gradient and workspace from torch.full inside ``guarded()``: guarded as well."""
    DB.case_resize_adjoint_is_exact_on_every_route(dlib, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("case", DR.RESIZE_BOUNDED, ids=DR.case_id)
def test_resize_adjoint_bounded_routes(guard, dlib, case):
    DB.case_resize_adjoint_at_other_ratios_within_the_counted_bound(dlib, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("case", DR.TAPSUM_CASES, ids=DR.case_id)
def test_tapsum_bwd(guard, dlib, case):
    DB.case_tapsum_bwd_is_exact(dlib, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("kind,case", [("disjoint", c) for c in DR.COL2IM_DISJOINT] + [("gather", c) for c in DR.COL2IM_GATHER],
                         ids=lambda v: v if isinstance(v, str) else DR.case_id(v))
def test_col2im(guard, dlib, kind, case):
    DB.case_col2im_is_exact(dlib, kind, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("case", DR.DWCONV_CASES, ids=DR.case_id)
def test_dwconv_forward_and_both_gradients(guard, dlib, case):
    DB.case_dwconv_forward_and_both_gradients_are_exact(dlib, case, up=guard.put)
    guard.finish(ws=True)


@pytest.mark.parametrize("case", DR.HEAD_CASES, ids=DR.case_id)
def test_head_bwd(guard, dlib, case):
    DB.case_head_bwd_is_exact(dlib, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("case", DR.CONV_IN_CASES, ids=DR.case_id)
def test_conv_in_bwd(guard, dlib, case):
    DB.case_conv_in_bwd_is_exact(dlib, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("swish", [False, True], ids=["exact", "swish"])
@pytest.mark.parametrize("case", DR.DENSE_CASES, ids=DR.case_id)
def test_dense_small_bwd(guard, dlib, case, swish):
    body = DB.case_dense_small_bwd_with_swish_within_the_measured_bound if swish else DB.case_dense_small_bwd_without_swish_is_exact
    body(dlib, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("case", DR.AUDIO_CASES, ids=DR.case_id)
def test_audio_fuse_and_its_backward(guard, dlib, case):
    DB.case_audio_fuse_and_its_backward_within_the_measured_bound(dlib, case, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("n", DR.MSE_NS)
@pytest.mark.parametrize("want_grad", [True, False])
def test_mse_loss(guard, dlib, n, want_grad):
    DB.case_mse_loss_value_within_the_counted_bound_and_gradient_exact(dlib, n, want_grad, up=guard.put)
    guard.finish(ws=True)


@pytest.mark.parametrize("n", DR.NORM_NS)
@pytest.mark.parametrize("spread", [False, True])
def test_grad_norm(guard, dlib, n, spread):
    DB.case_grad_norm_within_one_rounding(dlib, n, spread, up=guard.put)
    guard.finish(ws=True)


@pytest.mark.parametrize("case", TR.RELPOS_CASES, ids=TR.case_id)
def test_relpos_project_forward_and_backward(guard, elib, case):
    EN.case_relpos_project_forward_and_backward_are_exact(elib, case, up=guard.put)
    guard.finish(ws=True)


@pytest.mark.parametrize("D", TR.REL_DS)
@pytest.mark.parametrize("block", TR.REL_BLOCKS, ids=TR.case_id)
def test_rel_tables_forward_and_backward(guard, elib, block, D):
    EN.case_rel_tables_forward_backward_and_an_unused_table(elib, block, D, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("C", TR.MAXPOOL_CS)
@pytest.mark.parametrize("case", TR.MAXPOOL_CASES, ids=TR.case_id)
def test_maxpool_tokens_with_indices(guard, elib, case, C):
    EN.case_maxpool_ties_go_to_the_first_window_position(elib, case, C, up=guard.put)
    guard.finish()


@pytest.mark.parametrize("param_layout", (False, True), ids=("tap-major", "parameter-layout"))
def test_qkv_pool_per_tensor_route(guard, elib, param_layout):
    EN.case_qkv_pool_per_tensor_route(elib, param_layout, up=guard.put)
    guard.finish(ws=True)


@pytest.mark.parametrize("case", VR.GN_TRAIN, ids=VR.ids(VR.GN_TRAIN))
def test_groupnorm_swish_training(guard, agops, case):
    """rowstats, reduce_partials, norm_finalize_fwd / _bwd and norm_bwd_apply with their fp64 partial buffers between bands."""
    VR.case_groupnorm_swish_training(agops, case, up=guard.put)
    guard.finish(ws=True)


@pytest.mark.parametrize("case", VR.BN, ids=VR.ids(VR.BN))
def test_batchnorm_training(guard, agops, case):
    VR.case_batchnorm_training(agops, case, up=guard.put)
    guard.finish(ws=True)
