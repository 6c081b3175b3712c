"""The ctypes binding is derived from include/diffsal.h: the declaration reader on its own, then what _lib builds with it."""
import ctypes as C

import pytest

from diff_sal_amd import _cdecl, _lib, audio_input, ops
from diff_sal_amd import build as _build
from tests.test_abi import declared_symbols

SAMPLE = """
/* a comment with int diffsal_not_a_prototype(int x); inside */
#ifndef SAMPLE_H
#define SAMPLE_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* diffsal_stream_t; /* a handle */
#define DIFFSAL_ABI_VERSION 7
#define DIFFSAL_FLAG 4u
enum { DIFFSAL_OK = 0, DIFFSAL_E_SHAPE = -1,  /* between enumerators */
       DIFFSAL_TWO = 2 };
typedef struct diffsal_s {
  int Cout, Cin, taps;   /* several declarators */
  const float* p;
  long long rows;
} diffsal_s;
int diffsal_version(void);
const char* diffsal_name(void);
size_t diffsal_a(const diffsal_s* d /*host*/, const void* const* srcs, float* const* outs, int, const float*,
                 unsigned int terms, const unsigned long long* seed, unsigned char* u8, long long n, uint64_t s,
                 double e, long m, diffsal_stream_t stream);
long diffsal_set(const char* name, float const* x, const diffsal_s* const* many, int value);
#ifdef __cplusplus
}
#endif
#endif /* SAMPLE_H */
"""


def test_reader_forms():
    d = _cdecl.parse(SAMPLE)
    assert list(d.prototypes.items()) == [
        ("diffsal_version", ("int", [])),
        ("diffsal_name", ("const char*", [])),
        ("diffsal_a", ("size_t", ["const diffsal_s*", "const void* const*", "float* const*", "int", "const float*", "unsigned int",
                                  "const unsigned long long*", "unsigned char*", "long long", "uint64_t", "double", "long",
                                  "diffsal_stream_t"])),
        ("diffsal_set", ("long", ["const char*", "float const*", "const diffsal_s* const*", "int"])),
    ]
    assert d.structs == {"diffsal_s": [("Cout", "int"), ("Cin", "int"), ("taps", "int"), ("p", "const float*"), ("rows", "long long")]}
    assert d.constants == {"DIFFSAL_ABI_VERSION": 7, "DIFFSAL_FLAG": 4, "DIFFSAL_OK": 0, "DIFFSAL_E_SHAPE": -1, "DIFFSAL_TWO": 2}

    S = _cdecl.structure("S", d.structs["diffsal_s"], {"diffsal_s": None})
    assert S._fields_ == [("Cout", C.c_int), ("Cin", C.c_int), ("taps", C.c_int), ("p", C.c_void_p), ("rows", C.c_longlong)]
    structs = {"diffsal_s": S}
    assert [_cdecl.ctype(t, structs) for t in d.prototypes["diffsal_a"][1]] == [
        C.POINTER(S), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.c_longlong, C.c_uint64,
        C.c_double, C.c_long, C.c_void_p]
    assert [_cdecl.ctype(t, structs) for t in d.prototypes["diffsal_set"][1]] == [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int]
    assert [_cdecl.ctype(d.prototypes[n][0], structs) for n in d.prototypes] == [C.c_int, C.c_char_p, C.c_size_t, C.c_long]


@pytest.mark.parametrize("text", ["int diffsal_x(short a);", "int diffsal_x(struct foo* p);",
                                  "typedef struct diffsal_s { short a; } diffsal_s;"])
def test_reader_refuses_what_is_outside_its_vocabulary(text):
    with pytest.raises(ValueError):
        _cdecl.parse(text)


@pytest.mark.parametrize("text", ["short diffsal_x(void);", "int diffsal_x();", "int diffsal_x(int a,);", "int diffsal_x(diffsal_s s);",
                                  "enum { DIFFSAL_A, DIFFSAL_B = 1 };", "typedef struct diffsal_s { int a; } diffsal_t;",
                                  "typedef struct diffsal_s { float *a, *b; } diffsal_s;", "static int x = 3;"])
def test_reader_refuses_other_forms(text):
    with pytest.raises(ValueError):
        _cdecl.parse(text)


def test_whole_header():
    d = _cdecl.parse(open(_build.HEADER).read())
    assert len(d.prototypes) == len(declared_symbols()) >= 153      # 158 before the F(2x2) path and two forwarding entry points left
    assert list(_lib.SIGNATURES) == list(d.prototypes)      # header order
    structs = dict.fromkeys(d.structs)
    for name, (res, args) in d.prototypes.items():
        for t in [res] + args:
            assert issubclass(_cdecl.ctype(t, structs), (C._SimpleCData, C._Pointer)), (name, t)


def test_pinned_signatures():
    """The entries with the least common types, as the hand-written table had them (host arrays now travel as c_void_p)."""
    c_f, c_i, c_fl, c_sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    desc, ext = C.POINTER(_lib.ConvDesc), C.POINTER(_lib.Wino4Ext)
    expected = {
        "diffsal_adam_step": (c_i, [c_f, c_f, c_f, c_f, C.c_long, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, c_i,
                                    c_fl, c_f, c_fl, c_i, c_f]),
        "diffsal_eval_metrics": (c_i, [c_f, c_f, c_f, c_f, c_i, C.c_long, C.c_uint, c_i, C.c_double, c_f, c_f, c_i, c_f, c_f, c_f,
                                       c_sz, c_f, c_f]),
        "diffsal_attention_general_bwd": (c_i, [c_f] * 12 + [c_sz] + [c_f, c_sz] + [c_f] * 4 + [c_i] * 7 + [c_f] * 4
                                          + [c_fl, c_i, c_f]),
        "diffsal_dropout": (c_i, [c_f, c_f, c_sz, c_fl, C.c_uint64, c_f]),
        "diffsal_conv_wino4": (c_i, [desc] + [c_f] * 9 + [c_sz, ext, c_i, c_f]),
        "diffsal_resize_sum": (c_i, [c_f, c_f, c_f, c_i, c_f, c_i, c_i, c_i, c_i, c_i, c_f]),
        "diffsal_conv_igemm_group": (c_i, [c_i, c_f, c_f, c_f, c_f, c_f, c_f, c_sz, c_f]),
        "diffsal_tapsum_bwd_ws_bytes": (C.c_long, [c_i, c_i, c_i, c_i]),
        "diffsal_jpeg_capacity": (C.c_long, [c_i, c_i]),
        "diffsal_last_error": (C.c_char_p, []),
    }
    for name, sig in expected.items():
        assert _lib.SIGNATURES[name] == sig, name
    # one F(4x4) entry point with 14 parameters; the F(2x2) path and the forwarding entry points are gone
    assert len(_lib.SIGNATURES["diffsal_conv_wino4"][1]) == 14
    for gone in ("diffsal_conv_wino", "diffsal_conv_wino_supported", "diffsal_conv_wino_ws_bytes", "diffsal_conv_wino4_ex",
                 "diffsal_conv_wino4_stages"):
        assert gone not in _lib.SIGNATURES, gone


def test_struct_layouts():
    assert C.sizeof(_lib.ConvDesc) == 80
    assert _lib.ConvDesc._fields_ == [(n, C.c_int) for n in (
        "N", "H", "W", "Cin", "Ho", "Wo", "Cout", "KH", "KW", "stride_h", "stride_w", "pad_t", "pad_l", "dil_h", "dil_w", "act",
        "rowvec_ld", "w_format", "precision", "dtype")]

    assert C.sizeof(_lib.Wino4Ext) == 88
    pointers = ("in_ab", "side_a", "side_w", "side_out", "out_stats", "up2_c", "up2_scale", "up2_shift")
    ints = ("in_swish", "out_groups", "up2_act", "reserved")
    assert _lib.Wino4Ext._fields_ == ([(n, C.c_void_p) for n in pointers] + [("side_rows", C.c_longlong)]
                                      + [(n, C.c_int) for n in ints])
    assert [getattr(_lib.Wino4Ext, n).offset for n in pointers] == list(range(0, 64, 8))
    assert _lib.Wino4Ext.side_rows.offset == 64
    assert [getattr(_lib.Wino4Ext, n).offset for n in ints] == [72, 76, 80, 84]

    assert C.sizeof(_lib.PackJob) == 40
    assert [(n, getattr(_lib.PackJob, n).offset, getattr(_lib.PackJob, n).size) for n, _ in _lib.PackJob._fields_] == [
        ("src", 0, 8), ("dst", 8, 8), ("Cout", 16, 4), ("Cin", 20, 4), ("taps", 24, 4), ("mode", 28, 4), ("tile0", 32, 4),
        ("reserved", 36, 4)]


def test_constants():
    assert _lib.ABI_VERSION == 53
    assert (_lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_GELU, _lib.ACT_SIGMOID, _lib.ACT_GELU_GRAD) == (0, 1, 2, 3, 5)
    assert (ops.ACT_NONE, ops.ACT_RELU, ops.ACT_GELU, ops.ACT_SIGMOID, ops.ACT_GELU_GRAD) == (0, 1, 2, 3, 5)
    assert (_lib.PREC_FP32, _lib.PREC_BF16X3) == (0, 1)
    assert (_lib.F32, _lib.BF16, _lib.F16) == (0, 1, 2)
    assert (_lib.WS_GROUPNORM, _lib.WS_CONV_IGEMM, _lib.WS_CONV_WINO4, _lib.WS_CONV_WINO4_STATS,
            _lib.WS_CONV_WGRAD, _lib.WS_WGRAD_SEGMENTED, _lib.WS_TAPSUM_BWD, _lib.WS_SALIENCY_METRICS, _lib.WS_ATTENTION_TAIL,
            _lib.WS_ATTENTION_BWD_QTAIL, _lib.WS_ATTENTION_BWD_DS) == (0, 1) + tuple(range(3, 12))      # 2: retired with F(2x2)
    assert "DIFFSAL_WS_CONV_WINO" not in _lib.K
    assert (ops.EVAL_JUDD, ops.EVAL_BORJI, ops.EVAL_SAUC, ops.EVAL_CC, ops.EVAL_NSS, ops.EVAL_SIM, ops.EVAL_JITTER) == (
        1, 2, 4, 8, 16, 32, 64)
    assert (ops.FILTER_BILINEAR, ops.FILTER_BICUBIC) == (0, 1)
    assert (ops.RESAMPLE_AUTO, ops.RESAMPLE_FUSED, ops.RESAMPLE_TWO_PASS) == (0, 1, 2)
    import torch
    assert audio_input._WAV_DTYPES == {torch.int16: 0, torch.float32: 1, torch.float64: 2}
    assert (_lib.K["DIFFSAL_OK"], _lib.K["DIFFSAL_E_SHAPE"], _lib.K["DIFFSAL_E_ALIGN"], _lib.K["DIFFSAL_E_LAUNCH"],
            _lib.K["DIFFSAL_E_ARG"]) == (0, -1, -2, -3, -4)
    with pytest.raises(KeyError):
        _lib.constants("ACT_", "NONE NO_SUCH_NAME")


def test_missing_header_is_one_clear_error(tmp_path, monkeypatch):
    """Runs _lib's source as a scratch module (the imported _lib stays as it is) with the header path pointing nowhere."""
    import importlib.util

    monkeypatch.setattr(_build, "HEADER", str(tmp_path / "include" / "diffsal.h"))
    spec = importlib.util.spec_from_file_location("diff_sal_amd._lib_without_header", _lib.__file__)
    with pytest.raises(ImportError, match=str(tmp_path)):
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
