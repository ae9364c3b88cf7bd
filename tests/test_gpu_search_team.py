"""GPU: opt-in multi-wave search teams (vsg_index_set_search_team; csrc/hnsw_search_team.hip):
results and counters equal the one-wave register search's bit for bit on any data, and the
oracle's traversal of the same graph on integer data; search_team_queries tells the paths apart."""
import functools

import numpy as np
import pytest

import oracle as O
import vsg
from vsg import _lib
from vsg import datagen as G

pytestmark = pytest.mark.gpu

N = 6000
# (metric, dim, storage, M): 768-d rows; the 8 x 2 short-row shape; a ragged last chunk with
# full 64-entry adjacency pieces; 64-lane rows with M0 = 80 (two pieces, the second short)
SHAPES = [("cos", 768, "f32", 16), ("l2sq", 128, "f16", 16), ("ip", 100, "f32", 32), ("ip", 1536, "f32", 40)]
EF_K = [(10, 10), (64, 10), (65, 20), (192, 32)]


@functools.lru_cache(maxsize=None)
def built(metric, dim, quant, M, integer=False):  # (index, queries): clustered floats, or integers in 0..255
    if integer:
        x, q = G.uint8_valued(N, dim, 71), G.uint8_valued(130, dim, 72)
    else:
        bs, qs, ms = G.config_seeds(1)
        x, q = G.clustered(N, dim, bs, ms), G.clustered(130, dim, qs, ms)
        if metric == "ip":
            x /= np.linalg.norm(x, axis=1, keepdims=True)
            q /= np.linalg.norm(q, axis=1, keepdims=True)
    idx = vsg.Index(dim, metric, quant, M, 64, 48, seed=7)
    idx.add(np.arange(N), x)
    assert idx.graph_info()["max_level"] >= 1  # the greedy descent runs too
    return idx, q


def search(idx, q, k, ef, waves):
    s0 = idx.stats()
    idx.set_search_team(waves)
    m = idx.search(q, k, ef)
    idx.set_search_team(0)
    s1 = idx.stats()
    return (m.keys, m.distances, m.counts), [s1[f] - s0[f] for f in ("search_team_queries", "search_distances",
                                                                   "search_adjacency")]


def same(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("waves", [2, 4])
@pytest.mark.parametrize("metric,dim,quant,M", SHAPES)
def test_team_walk_equals_one_wave_walk(metric, dim, quant, M, waves):
    idx, q = built(metric, dim, quant, M)
    for nq in (1, 3, 130):
        for ef, k in EF_K:
            ref, d0 = search(idx, q[:nq], k, ef, 0)
            got, d1 = search(idx, q[:nq], k, ef, waves)
            same(got, ref)
            assert d0[0] == 0 and d1[0] == nq and d1[1:] == d0[1:], (nq, ef, d0, d1)


@pytest.mark.parametrize("metric,dim,quant,M", [SHAPES[1], SHAPES[2]])
def test_team_walk_equals_oracle_on_integer_data(metric, dim, quant, M):
    """Values in 0..255: every partial sum is an integer below 2^24, so distances are exact."""
    idx, q = built(metric, dim, quant, M, integer=True)
    h = O.HnswOracle(dim, metric, M, 64, 48, seed=7)
    h.import_graph(idx.export())
    for ef, k in EF_K:
        got, d = search(idx, q, k, ef, 4)
        assert d[0] == len(q)
        same(got, h.search(q, k, ef))


def test_team_fallbacks_and_setter_contract(monkeypatch):
    idx, q = built("ip", 100, "f32", 32)
    for waves, code, make in ((3, _lib.VSG_EINVAL, lambda: idx), (8, _lib.VSG_EINVAL, lambda: idx),
                              (2, _lib.VSG_EUNSUPPORTED, lambda: vsg.Index(32, "l2sq", "f32", exact_only=True))):
        with pytest.raises(vsg.VsgError) as e:
            make().set_search_team(waves)
        assert e.value.code == code

    def falls_back(i, qq, k, ef):
        ref, _ = search(i, qq, k, ef, 0)
        got, d = search(i, qq, k, ef, 4)
        same(got, ref)
        assert d[0] == 0

    falls_back(idx, q, 10, 193)  # above the 4-row register class
    monkeypatch.setenv("VSG_SEARCH_TEAM_MAX_QUERIES", "2")
    falls_back(idx, q[:3], 10, 48)  # more teams than are resident at once
    monkeypatch.delenv("VSG_SEARCH_TEAM_MAX_QUERIES")
    for mode in (idx.set_i8_traversal, idx.set_f16_traversal):
        mode(True)
        falls_back(idx, q, 10, 48)
        mode(False)
    # a fresh index: the environment variable decides until the setter is called; removed entries
    x = G.uint8_valued(N, 64, 81)
    env = vsg.Index(64, "l2sq", "f32", 16, 64, 48, seed=7)
    env.add(np.arange(N), x)
    ref = env.search(x[:50], 10, 48)
    monkeypatch.setenv("VSG_SEARCH_TEAM", "4")
    got = env.search(x[:50], 10, 48)
    same((got.keys, got.distances, got.counts), (ref.keys, ref.distances, ref.counts))
    assert env.stats()["search_team_queries"] == 50
    env.remove(np.arange(0, N, 9))
    falls_back(env, x[:50], 10, 48)
