"""bf16 storage (VSG_SCALAR_BF16): rows and queries rounded to bf16 (nearest, ties to even),
every distance accumulated in f32.  Integer data of <= 8 significant bits is exact in bf16,
so the oracle (which knows no quantisation) pins exact search, graph search and build bit
for bit; float data pins the rounding itself and the f32 accumulation of the matrix cores.
"""
import numpy as np
import pytest

import oracle as O
import vsg
from vsg import datagen as G

pytestmark = pytest.mark.gpu

N = 6000
EF_K = [(10, 10), (64, 10), (192, 32), (1100, 10)]  # 2- and 4-row register sets, the LDS list


def ints(n, dim, seed, metric, hi=256):
    """Integers in [0, hi) (ip: sixteenths): every partial sum stays below 2^24 -- l2sq
    dim * (hi - 1)^2 <= 12.4 M for (128, 256) and (768, 128); ip in units of 1/256 at most
    9.7 M for the 520-d rows used here (checked in float64 when the shapes were chosen)."""
    x = np.floor(G.uint8_valued(n, dim, seed) * (hi / 256.0)).astype(np.float32)
    return x / 16.0 if metric == "ip" else x


def rne_bf16(a):
    """Round-to-nearest-even of f32 to bf16, widened again, stated on the uint32 view."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    r = np.where((u & 0x7FFFFFFF) > 0x7F800000, (u & 0xFFFF0000) | 0x00400000, r)  # NaN stays NaN
    return r.astype(np.uint32).view(np.float32)


def counted(idx, field, call):
    before = idx.stats()[field]
    m = call()
    return (m.keys, m.distances, m.counts), idx.stats()[field] - before


def same(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("metric,dim,n,nq,k,cores", [
    ("l2sq", 64, 700, 31, 10, False),   # VALU: batch below 32
    ("ip", 520, 700, 40, 10, False),    # VALU: rows that are no whole 32-element groups
    ("l2sq", 128, 3001, 33, 10, True),  # two stages, ragged row tile, the 64-query tile
    ("ip", 96, 5000, 200, 16, True),    # one and a half stages, two query tiles, full k
    ("l2sq", 32, 130, 40, 7, True),     # only a half stage, fewer rows than a tile
    ("ip", 96, 4099, 33, 17, True),     # wide-k: its smallest k, a half stage
    ("l2sq", 128, 4099, 33, 100, True),  # wide-k
])
def test_exact_search_bitexact_integer(metric, dim, n, nq, k, cores, monkeypatch):
    x, q = ints(n, dim, 81, metric), ints(nq, dim, 82, metric)
    keys = np.arange(n, dtype=np.uint64) * 3 + 11
    removed = np.zeros(n, np.uint8)
    removed[::7] = 1
    idx = vsg.Index(dim, metric, "bf16")
    idx.add(keys, x)
    idx.remove(keys[::7])
    ref = O.exact_search(metric, x, q, k, keys=keys, removed=removed)
    for env in ("1", "0"):
        monkeypatch.setenv("VSG_EXACT_MFMA", env)
        got, moved = counted(idx, "exact_mfma_queries", lambda: idx.exact_search(q, k))
        assert moved == (nq if cores and env == "1" else 0)
        same(got, ref)


@pytest.mark.parametrize("metric,dim,extra", [("l2sq", 128, "remove"),  # 16 chunks
                                              ("ip", 100, "team"),       # 13 chunks, ragged last chunk
                                              ("l2sq", 768, None)])      # 96 chunks: 32 lanes x 3
def test_graph_search_equals_oracle_walk(metric, dim, extra):
    hi = 128 if dim == 768 else 256
    x, q = ints(N, dim, 71, metric, hi), ints(64, dim, 72, metric, hi)
    idx = vsg.Index(dim, metric, "bf16", 16, 64, 48, seed=7)
    idx.add(np.arange(N), x)
    assert idx.graph_info()["max_level"] >= 1  # the greedy descent runs too
    idx.set_search_team(4 if extra == "team" else 0)
    for step in ("built", "remove")[:2 if extra == "remove" else 1]:
        if step == "remove":
            idx.remove(np.arange(0, N, 9))  # the filtered search
        h = O.HnswOracle(dim, metric, 16, 64, 48, seed=7)
        h.import_graph(idx.export())
        for ef, k in EF_K:
            got, teams = counted(idx, "search_team_queries", lambda: idx.search(q, k, ef))
            assert teams == (len(q) if extra == "team" and ef <= 192 else 0)
            same(got, h.search(q, k, ef))


@pytest.mark.parametrize("metric,dim,efc", [("ip", 48, 128), ("l2sq", 768, 64)])
def test_one_node_batches_build_the_oracle_graph(metric, dim, efc, monkeypatch):
    """test_hnsw_gpu_build_one_node_batches_equals_oracle_graph on bf16 rows."""
    n = 1500
    x = ints(n, dim, 33, metric, 128 if dim == 768 else 256)
    monkeypatch.setenv("VSG_BUILD_PERMUTE", "0")
    monkeypatch.setenv("VSG_BUILD_BATCH_MAX", "1")
    gpu = vsg.Index(dim, metric, "bf16", 16, efc, 64, seed=21)
    gpu.add(np.arange(n), x)
    h = O.HnswOracle(dim, metric, 16, efc, 64, seed=21)
    h.add(np.arange(n), x, threads=1)
    a, b = gpu.export(), h.export()
    assert (a["entry"], a["max_level"]) == (b["entry"], b["max_level"])
    for key in ("levels", "upper_off", "adj0", "upper"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def test_rounding_contract():
    bits = lambda *w: np.array(w, np.uint32).view(np.float32)  # noqa: E731
    # lost by f16; near the top; beyond the largest bf16; ties with an even and an odd kept
    # bit, just above and below a tie; NaN with its payload in the dropped half only; inf
    row = np.concatenate([np.array([1e5, 1e-6, 3.0e38, 3.4e38, np.inf, 0.0], np.float32),
                          bits(0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0x7F800001, 0x7FC00000)])
    x = np.stack([row, -row, row[::-1], np.full(12, 0.1, np.float32)])
    idx = vsg.Index(12, "ip", "bf16", exact_only=True)
    idx.add(np.arange(4), x)
    got = idx.export()["vectors"]
    np.testing.assert_array_equal(got.view(np.uint32), rne_bf16(x).view(np.uint32))
    # the statement itself, where it matters
    assert got[0, 0] == 99840.0 and 0.99e-6 < got[0, 1] < 1.01e-6 and np.isfinite(got[0, 2]) and got[0, 3] == np.inf
    assert got[0, 6:10].view(np.uint32).tolist() == [0x3F800000, 0x3F820000, 0x3F810000, 0x3F810000]
    assert np.isnan(got[0, 10:]).all() and np.isnan(got[1, 10:]).all() and got[1, 4] == -np.inf


@pytest.mark.parametrize("metric,dim", [("ip", 256), ("l2sq", 768), ("cos", 768)])
def test_float_distances_vs_float64(metric, dim, monkeypatch):
    """float64 over the exported rows and the queries rounded the same way; the bar of
    test_exact_float_golden (bf16 x bf16 products are exact in f32: only the f32 accumulation
    is in it).  k 10: the register-list kernel, k 100: the wide-k kernel, whose 4,096-row
    threshold is lowered to these 4,000 rows."""
    n, nq = 4000, 150
    monkeypatch.setenv("VSG_EXACT_WIDE_MIN_ROWS", str(n))
    bs, qs, ms = G.config_seeds(4)
    q = G.clustered(nq, dim, qs, ms)
    idx = vsg.Index(dim, metric, "bf16")
    idx.add(np.arange(n), G.clustered(n, dim, bs, ms))
    xs = idx.export()["vectors"].astype(np.float64)
    qn = q / np.sqrt(np.sum(q * q, axis=1, dtype=np.float32))[:, None] if metric == "cos" else q
    qr = rne_bf16(qn).astype(np.float64)
    if metric == "l2sq":
        ref = (xs * xs).sum(1)[None, :] + (qr * qr).sum(1)[:, None] - 2.0 * qr @ xs.T
    else:
        ref = 1.0 - qr @ xs.T
    order = np.argsort(ref, axis=1, kind="stable")
    rd = np.take_along_axis(ref, order, axis=1)
    for k in (10, 100):
        (keys, dist, _), moved = counted(idx, "exact_mfma_queries", lambda: idx.exact_search(q, k))
        assert moved == nq
        err = np.abs(dist - rd[:, :k]) / np.maximum(1.0, np.abs(rd[:, :k]))
        print(f"{metric}-{dim} k {k}: max relative distance error {err.max():.3e}")
        assert err.max() < 1e-4
        for i in range(nq):
            if set(keys[i].tolist()) != set(order[i, :k].tolist()):
                assert rd[i, k] - rd[i, k - 1] < 1e-4


def test_recall_parity_with_f32():
    """Each index against exact search over its own stored rows: storage precision does not
    enter, the bar is the f16 / int8 walk tests' 0.01."""
    bs, qs, ms = G.config_seeds(1)
    x, q = G.clustered(N, 768, bs, ms), G.clustered(130, 768, qs, ms)
    rec = {}
    for quant in ("f32", "bf16"):
        idx = vsg.Index(768, "cos", quant, 16, 64, 48, seed=7)
        idx.add(np.arange(N), x)
        truth = idx.exact_search(q, 10).keys
        rec[quant] = [np.mean([len(set(a) & set(b)) / 10 for a, b in zip(idx.search(q, 10, ef).keys, truth)])
                      for ef in (16, 64)]
    print(f"recall@10 at ef 16 / 64: f32 {rec['f32']}, bf16 {rec['bf16']}")
    assert all(b >= f - 0.01 for b, f in zip(rec["bf16"], rec["f32"]))


def test_life_cycle(tmp_path):
    metric, dim, n = "l2sq", 128, 3000
    x, q = ints(n, dim, 91, metric), ints(40, dim, 92, metric)
    keys = np.arange(n, dtype=np.uint64) * 3 + 11
    new = lambda quant="bf16": vsg.Index(dim, metric, quant, 16, 64, 48, seed=7)  # noqa: E731
    a = new()
    a.add(keys, x)
    a.save(tmp_path / "a.vsg")
    assert vsg.file_info(tmp_path / "a.vsg")["quantization"] == "bf16"
    loaded, imported = vsg.Index.load(tmp_path / "a.vsg"), new()
    imported.import_graph(a.export())
    answers = lambda i: [getattr(m, f) for m in (i.search(q, 10, 48), i.exact_search(q, 10))  # noqa: E731
                         for f in ("keys", "distances", "counts")]
    assert loaded.quantization == "bf16"
    for other in (loaded, imported):
        same(answers(other), answers(a))
    sh = vsg.ShardedIndex(dim, metric, "bf16", 16, 64, 48, devices=[0, 0], seed=7)
    sh.add(keys, x)
    m = sh.exact_search(q, 10)
    same((m.keys, m.distances), O.exact_search(metric, x, q, 10, keys=keys)[:2])
    # the f32-only modes: what an f16 index does -- the error code, or the silent non-use
    f16 = new("f16")
    f16.add(keys, x)
    for mode in ("set_f16_traversal", "set_i8_traversal", "set_prefilter"):
        outcome = []
        for i in (a, f16):
            try:
                getattr(i, mode)(True)
                i.search(q, 10, 48)
                outcome.append([i.stats()[f] for f in ("search_sketch_rows", "search_i8_queries")])
            except vsg.VsgError as e:
                outcome.append(e.code)
        assert outcome[0] == outcome[1], (mode, outcome)
