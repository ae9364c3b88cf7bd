"""Exact search with 17 <= k <= 128 on the matrix cores (csrc/mfma_exact_wide.hip): batches
of >= 32 queries over >= 4,096 rows of whole 32-element groups, either storage.
vsg_stats_t.exact_mfma_queries says which kernel answered."""
import numpy as np
import pytest

import oracle as O
import vsg
from vsg import datagen as G

pytestmark = pytest.mark.gpu


def integer_case(metric, dim, n, nq, quant, shape="plain"):
    """uint8-valued rows (exact in f16, every sum below 2^24), keys 3 i + 11, every 7th removed."""
    scale = 16.0 if metric == "ip" else 1.0
    x = G.uint8_valued(n, dim, 81) / scale
    q = G.uint8_valued(nq, dim, 82) / scale
    removed = np.zeros(n, np.uint8)
    removed[::7] = 1
    if shape == "twice":  # every distance ties across tiles and splits: the slot decides
        x[n // 2:] = x[:n - n // 2]
    elif shape == "descending":  # |x|^2 strictly falls with the slot: every row survives tau
        v = n - 1 - np.arange(n)
        col = np.arange(dim)[None, :]
        x = np.where(col < (v // 255)[:, None], 255, np.where(col == (v // 255)[:, None], (v % 255)[:, None], 0))
        x = x.astype(np.float32)
        q = (G.uint8_valued(nq, dim, 82) % 4).astype(np.float32)
    elif shape == "sparse":  # 100 live rows < k
        removed[:] = 1
        removed[np.arange(100) * 41 + 5] = 0
    keys = np.arange(n, dtype=np.uint64) * 3 + 11
    idx = vsg.Index(dim, metric, quant)
    idx.add(keys, x)
    idx.remove(keys[removed == 1])
    return idx, x, q, keys, removed


def counted_search(idx, q, k):
    before = idx.stats()["exact_mfma_queries"]
    m = idx.exact_search(q, k)
    return m, idx.stats()["exact_mfma_queries"] - before


def assert_equal(m, ref):
    for got, want in zip((m.keys, m.distances, m.counts), ref):
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("quant", ["f32", "f16"])
@pytest.mark.parametrize("metric,dim,n,nq,k,splits,shape", [
    ("l2sq", 32, 4099, 33, 17, None, "plain"),      # smallest k, ragged last tile, f16 half stage, splits < k rows
    ("ip", 96, 5000, 200, 100, None, "plain"),      # k no power of two, two query tiles, 1.5 f16 stages
    ("l2sq", 128, 5000, 257, 128, 2, "plain"),      # largest k, three query tiles, 20 tiles per split
    ("l2sq", 128, 5000, 257, 128, 2, "twice"),      # ties across tiles and across the two splits
    ("l2sq", 128, 5000, 257, 128, 2, "descending"),  # the pool fills to its capacity
    ("l2sq", 64, 4200, 40, 128, None, "sparse"),    # counts = 100 < k: padding through pool, list, merge
])
def test_wide_bitexact_integer(quant, metric, dim, n, nq, k, splits, shape, monkeypatch):
    if splits:
        monkeypatch.setenv("VSG_EXACT_WIDE_SPLITS", str(splits))
    idx, x, q, keys, removed = integer_case(metric, dim, n, nq, quant, shape)
    ref = O.exact_search(metric, x, q, k, keys=keys, removed=removed)
    monkeypatch.setenv("VSG_EXACT_MFMA", "1")
    m, moved = counted_search(idx, q, k)
    assert moved == nq
    assert_equal(m, ref)
    monkeypatch.setenv("VSG_EXACT_MFMA", "0")
    v, moved = counted_search(idx, q, k)
    assert moved == 0
    assert_equal(v, ref)


@pytest.mark.parametrize("k,n,nq,dim", [(129, 5000, 40, 64), (17, 4095, 40, 64), (17, 5000, 31, 64), (100, 5000, 40, 520)])
def test_wide_dispatch_edges(k, n, nq, dim):
    idx, x, q, keys, removed = integer_case("l2sq" if dim == 64 else "ip", dim, n, nq, "f16")
    m, moved = counted_search(idx, q, k)
    assert moved == 0
    assert_equal(m, O.exact_search(idx.metric, x, q, k, keys=keys, removed=removed))


@pytest.mark.parametrize("metric,dim,quant", [("ip", 256, "f16"), ("l2sq", 768, "f32"), ("cos", 768, "f32")])
def test_wide_float_vs_float64(metric, dim, quant, monkeypatch):
    """float64 over the exported rows (f16: queries rounded as prepare_kernel rounds them)."""
    n, nq, k = 6000, 150, 100
    monkeypatch.setenv("VSG_EXACT_WIDE_SPLITS", "2")
    bs, qs, ms = G.config_seeds(4)
    q = G.clustered(nq, dim, qs, ms)
    idx = vsg.Index(dim, metric, quant)
    idx.add(np.arange(n), G.clustered(n, dim, bs, ms))
    m, moved = counted_search(idx, q, k)
    assert moved == nq
    xs = idx.export()["vectors"].astype(np.float64)
    if metric == "cos":
        q = q / np.sqrt(np.sum(q * q, axis=1, dtype=np.float32))[:, None]
    qr = (q.astype(np.float16) if quant == "f16" else q.astype(np.float32)).astype(np.float64)
    if metric == "l2sq":
        ref = (xs * xs).sum(1)[None, :] + (qr * qr).sum(1)[:, None] - 2.0 * qr @ xs.T
    else:
        ref = 1.0 - qr @ xs.T
    order = np.argsort(ref, axis=1, kind="stable")[:, :k + 1]
    rd = np.take_along_axis(ref, order, axis=1)
    err = np.abs(m.distances - rd[:, :k]) / np.maximum(1.0, np.abs(rd[:, :k]))
    print(f"{metric}-{dim}-{quant}: max relative distance error {err.max():.3e}")
    assert err.max() < 1e-4
    for i in range(nq):
        if set(m.keys[i].tolist()) != set(order[i, :k].tolist()):
            assert rd[i, k] - rd[i, k - 1] < 1e-4


def test_wide_rows_added_in_two_calls():
    x = G.uint8_valued(6000, 128, 91)
    q = G.uint8_valued(48, 128, 92)
    idx = vsg.Index(128, "l2sq", "f16")
    for beg, end in ((0, 4500), (4500, 6000)):  # a ragged tile, then rows appended behind it
        idx.add(np.arange(beg, end), x[beg:end])
        m, moved = counted_search(idx, q, 40)
        assert moved == 48
        assert_equal(m, O.exact_search("l2sq", x[:end], q, 40))
