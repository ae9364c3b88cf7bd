"""Exact search of an f16 index on the f16 matrix cores (csrc/mfma_exact_f16.hip): batches
of >= 32 queries with k <= 16 over rows of whole 32-half groups; everything else stays on
the VALU kernel.  vsg_stats_t.exact_mfma_queries says which kernel answered.
"""
import numpy as np
import pytest

import oracle as O
import vsg
from vsg import datagen as G

pytestmark = pytest.mark.gpu


def integer_case(metric, dim, n, nq):
    """uint8-valued rows (exact in f16, every sum below 2^24), keys 3 i + 11, every 7th removed."""
    scale = 16.0 if metric == "ip" else 1.0
    x = G.uint8_valued(n, dim, 81) / scale
    q = G.uint8_valued(nq, dim, 82) / scale
    keys = np.arange(n, dtype=np.uint64) * 3 + 11
    removed = np.zeros(n, np.uint8)
    removed[::7] = 1
    idx = vsg.Index(dim, metric, "f16")
    idx.add(keys, x)
    idx.remove(keys[::7])
    return idx, x, q, keys, removed


def counted_search(idx, q, k):
    before = idx.stats()["exact_mfma_queries"]
    m = idx.exact_search(q, k)
    return m, idx.stats()["exact_mfma_queries"] - before


def assert_equal(m, ref):
    for got, want in zip((m.keys, m.distances, m.counts), ref):
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("metric,dim,n,nq,k", [
    ("l2sq", 128, 3001, 33, 10),  # two stages, ragged row tiles, the <= 64-query tile
    ("ip", 96, 5000, 200, 16),    # one and a half stages, two query tiles, full k
    ("l2sq", 32, 130, 40, 7),     # only a half stage, fewer rows than one tile
    ("ip", 64, 1000, 257, 1),     # three query tiles, the last holding one query
])
def test_f16_mfma_bitexact_integer(metric, dim, n, nq, k, monkeypatch):
    idx, x, q, keys, removed = integer_case(metric, dim, n, nq)
    ref = O.exact_search(metric, x, q, k, keys=keys, removed=removed)
    monkeypatch.setenv("VSG_EXACT_MFMA", "1")
    m, moved = counted_search(idx, q, k)
    assert moved == nq
    assert_equal(m, ref)
    monkeypatch.setenv("VSG_EXACT_MFMA", "0")
    v, moved = counted_search(idx, q, k)
    assert moved == 0
    assert_equal(v, ref)


@pytest.mark.parametrize("metric,dim", [("ip", 256), ("l2sq", 768), ("cos", 768)])
def test_f16_mfma_float_vs_float64(metric, dim):
    """float64 distances over the stored f16 rows and the queries rounded as prepare_kernel
    rounds them; the bar of test_exact_float_golden."""
    n, nq, k = 4000, 150, 10
    bs, qs, ms = G.config_seeds(4)
    q = G.clustered(nq, dim, qs, ms)
    idx = vsg.Index(dim, metric, "f16")
    idx.add(np.arange(n), G.clustered(n, dim, bs, ms))
    m, moved = counted_search(idx, q, k)
    assert moved == nq
    xs = idx.export()["vectors"].astype(np.float64)
    if metric == "cos":
        q = q / np.sqrt(np.sum(q * q, axis=1, dtype=np.float32))[:, None]
    qr = q.astype(np.float16).astype(np.float64)
    if metric == "l2sq":
        ref = (xs * xs).sum(1)[None, :] + (qr * qr).sum(1)[:, None] - 2.0 * qr @ xs.T
    else:
        ref = 1.0 - qr @ xs.T
    order = np.argsort(ref, axis=1, kind="stable")[:, :k + 1]
    rd = np.take_along_axis(ref, order, axis=1)
    err = np.abs(m.distances - rd[:, :k]) / np.maximum(1.0, np.abs(rd[:, :k]))
    print(f"{metric}-{dim}: max relative distance error {err.max():.3e}")
    assert err.max() < 1e-4
    for i in range(nq):
        if set(m.keys[i].tolist()) != set(order[i, :k].tolist()):
            assert rd[i, k] - rd[i, k - 1] < 1e-4


@pytest.mark.parametrize("dim,nq,k", [(64, 40, 17), (64, 31, 10), (520, 40, 10)])
def test_f16_dispatch_edges_stay_on_valu(dim, nq, k):
    idx, x, q, keys, removed = integer_case("l2sq" if dim == 64 else "ip", dim, 700, nq)
    m, moved = counted_search(idx, q, k)
    assert moved == 0
    assert_equal(m, O.exact_search(idx.metric, x, q, k, keys=keys, removed=removed))


def test_f16_mfma_rows_added_in_two_calls():
    x = G.uint8_valued(700, 128, 91)
    q = G.uint8_valued(48, 128, 92)
    idx = vsg.Index(128, "l2sq", "f16")
    for beg, end in ((0, 300), (300, 700)):  # a ragged tile, then rows appended behind it
        idx.add(np.arange(beg, end), x[beg:end])
        m, moved = counted_search(idx, q, 10)
        assert moved == 48
        assert_equal(m, O.exact_search("l2sq", x[:end], q, 10))
