"""Benchmark post-processing without a GPU: the NumPy restatement (tests/_postprocess_ref.py) against the fixtures recorded from
numpy, PIL, matplotlib and scipy (tools/gen_postprocess_golden.py), against scipy directly where it imports, and the argument
checks of the C ABI, which precede any launch.

Bars.  Bytes and PNG floats: exact.  float64 resize: |d| <= 1e-12 -- fp64 epsilon 1.1e-16 x an l1 gain of 3 of the coefficient
filter per axis x 16 taps is about 1e-14; 1e-12 leaves two decimal digits for the order of summation.  CC, NSS, SIM rows: 1e-9,
the bar of test_gpu_eval_metrics.py."""
import numpy as np
import pytest

from diff_sal_amd import _lib
from tests import _eval_metrics_ref as mref
from tests import _postprocess_ref as ref

CASES = ref.load_cases()
F64_BAR, MOMENT_BAR = 1e-12, 1e-9


def _pred(name):
    return ref.big_input() if name == "big" else CASES[name]["pred"]


def _pick(a, c):
    return a[c["rows"]][:, c["cols"]]


def test_fixture_cases_are_the_ones_the_checks_need():
    shapes = {n: (tuple(_pred(n).shape), c["size"]) for n, c in CASES.items()}
    assert shapes == {"s4x5": ((2, 4, 5), (5, 9)), "s7x12": ((2, 7, 12), (11, 20)), "s2x3": ((1, 2, 3), (2, 7)),
                      "s33x70": ((3, 33, 70), (67, 131)), "big": ((2, 224, 384), (360, 640))}
    flat = CASES["s33x70"]["pred"][1]
    assert flat.min() == flat.max()                                                  # a flat image among non-flat neighbours
    for n, c in CASES.items():
        for b, p in enumerate(_pred(n)):
            if p.min() == p.max():
                continue
            assert len(np.unique(p)) < p.size or p.size <= 6, (n, b)                   # exact repeats: ties
    z = CASES["s7x12"]["zoom3_f64"]
    assert z.min() < 0.0 and z.max() > 1.0                                           # cubic overshoot on both sides before the clip
    c = CASES["s7x12"]["clip3_f64"]
    assert c.min() == 0.0 and c.max() == 1.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_bytes_and_png_floats_are_exact(name):
    c = CASES[name]
    pred = _pred(name)
    sub = (slice(None, None, 7), slice(None, None, 5)) if name == "big" else (slice(None), slice(None))
    for b in range(pred.shape[0]):
        q = ref.to_uint8(pred[b])
        assert q.dtype == np.uint8 and np.array_equal(q[sub], c["u8"][b])
        f = ref.from_uint8(q)
        assert f.dtype == np.float32 and np.array_equal(f[sub], c["imread"][b])
    if name == "s33x70":
        assert not c["u8"][1].any() and c["u8"][0].max() == 255 and c["u8"][2].min() == 0


@pytest.mark.parametrize("order", ref.ORDERS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_resize_equals_the_scipy_fixtures(name, order):
    c = CASES[name]
    pred = _pred(name)
    worst = 0.0
    for b in range(pred.shape[0]):
        m = ref.from_uint8(ref.to_uint8(pred[b]))
        for clip, key in ((False, "zoom"), (True, "clip")):
            got = _pick(ref.resize(m, c["size"], order=order, clip=clip), c)
            d = float(np.abs(got - c[f"{key}{order}_f64"][b]).max())
            worst = max(worst, d)
            assert d <= F64_BAR, (name, order, b, key, d)
            # scipy's float32 output is its float64 result rounded once; the restatement's rounding may differ where the two
            # float64 values straddle a rounding boundary, by one float32 step at most
            d32 = np.abs(got.astype(np.float32).astype(np.float64) - c[f"{key}{order}_f32"][b].astype(np.float64)).max()
            assert d32 <= 2.0 ** -23, (name, order, b, key, d32)      # one float32 step below 2
    print(f"{name} order {order}: worst |d| = {worst:.2e}")


def test_restatement_equals_scipy_directly():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for (h, w), (H, W) in (((4, 5), (5, 9)), ((2, 3), (2, 7)), ((9, 40), (9, 41)), ((33, 70), (67, 131))):
        x = rng.random((h, w), dtype=np.float32)
        for order in ref.ORDERS:
            want = ndimage.zoom(x.astype(np.float64), (H / h, W / w), order=order, mode="mirror", grid_mode=True)
            got = ref.resize(x, (H, W), order=order, clip=False)
            d = float(np.abs(got - want).max())
            print(f"{h} x {w} -> {H} x {W} order {order}: |d| = {d:.2e}")
            assert got.shape == want.shape and d <= F64_BAR


@pytest.mark.parametrize("name", ["s7x12", "s33x70"])
def test_metric_rows_of_the_restatement_maps(name):
    """CC, NSS and SIM are smooth in the map: the restatement's float32 maps give the recorded rows.  AUC-Judd counts ranks, which a
    last-bit difference in one pixel may move: it is asserted only where the restatement's float32 map equals scipy's bit for bit
    at every recorded point, and printed otherwise."""
    c = CASES[name]
    for b in range(c["pred"].shape[0]):
        m = ref.from_uint8(ref.to_uint8(c["pred"][b]))
        m3 = ref.resize(m, c["size"], order=3).astype(np.float32)
        m1 = ref.resize(m, c["size"], order=1).astype(np.float32)
        rows = {"auc_judd": mref.auc_judd(m3, c["fix"][b]), "nss": mref.nss(m1, c["fix"][b])}
        flat = not m.max() > m.min()
        rows["cc"] = float("nan") if flat else mref.cc(m3, c["gt"][b])
        rows["sim"] = float("nan") if flat else mref.sim(m3, c["gt"][b])
        same = np.array_equal(_pick(m3, c), c["clip3_f32"][b])
        for k, got in rows.items():
            want = float(c["expected"][k][b])
            print(f"{name}[{b}] {k}: {got!r} want {want!r} (float32 maps bit-equal at the recorded points: {same})")
            if np.isnan(want):
                assert np.isnan(got), (k, b)
            elif k != "auc_judd":
                assert abs(got - want) <= MOMENT_BAR, (k, b, got, want)
            elif same:
                assert abs(got - want) <= 1e-12, (k, b, got, want)


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.load()
    P = 256      # never dereferenced: every check precedes the first launch

    def resize(h, w, H, W, order, B=1, clip=1, f64=0):
        return lib.diffsal_map_resize(P, B, h, w, H, W, order, clip, f64, P, P, 1 << 30, None)

    assert resize(8, 8, 7, 9, 3) == -1 and b"shrinks an axis" in lib.diffsal_last_error()            # a downscale
    assert resize(8, 8, 9, 7, 1) == -1 and b"shrinks an axis" in lib.diffsal_last_error()
    assert resize(1, 8, 4, 9, 3) == -1 and b"at least 2 samples" in lib.diffsal_last_error()         # n < 2
    assert resize(8, 1, 9, 4, 1) == -1 and b"at least 2 samples" in lib.diffsal_last_error()
    for order in (0, 2, 4, 5):
        assert resize(8, 8, 9, 9, order) == -4 and b"order" in lib.diffsal_last_error()                # a bad order
    assert resize(8, 8, 9, 9, 3, clip=2) == -4 and resize(8, 8, 9, 9, 3, f64=7) == -4
    assert resize(8, 8, 9, 9, 3, B=0) == -1 and resize(8, 8, 9, 40000, 3) == -1
    assert lib.diffsal_map_resize(None, 1, 8, 8, 9, 9, 3, 1, 0, P, P, 1 << 30, None) == -4             # null input
    assert lib.diffsal_map_resize(P, 1, 8, 8, 9, 9, 3, 1, 0, P, P, 16, None) == -4 and b"workspace" in lib.diffsal_last_error()
    assert lib.diffsal_map_to_u8(None, 1, 64, P, None, P, 1 << 20, None) == -4
    assert lib.diffsal_map_to_u8(P, 1, 64, None, None, P, 1 << 20, None) == -4                          # no output asked for
    assert lib.diffsal_map_to_u8(P, 0, 64, P, None, P, 1 << 20, None) == -1
    assert lib.diffsal_map_to_u8(P, 1, 64, P, None, P, 0, None) == -4 and b"workspace" in lib.diffsal_last_error()
    assert lib.diffsal_map_from_u8(P, 0, P, None) == -1 and lib.diffsal_map_from_u8(None, 4, P, None) == -4
    # workspace sizes: order 3 keeps two [B][h][w] float64 arrays, the clip two floats per 4096-pixel chunk; host arithmetic only
    n, B = 224 * 384, 64
    part = (B * 21 * 2 * 4 + 15) // 16 * 16
    assert lib.diffsal_map_to_u8_ws_bytes(B, n) == part
    assert lib.diffsal_map_resize_ws_bytes(B, 224, 384, 3, 1) == part + 2 * B * n * 8
    assert lib.diffsal_map_resize_ws_bytes(B, 224, 384, 3, 0) == 2 * B * n * 8
    assert lib.diffsal_map_resize_ws_bytes(B, 224, 384, 1, 0) == 0 and lib.diffsal_map_resize_ws_bytes(B, 224, 384, 2, 0) == 0
