"""FP8 storage (VSG_SCALAR_F8, OCP E4M3) for exact-only indexes: rows and queries rounded to
E4M3 (nearest, ties to even, saturating at 448), every distance accumulated in f32.  Integers
of magnitude <= 8 are exact in E4M3, so the oracle (which knows no quantisation) pins both
exact kernels bit for bit; float data pins the rounding (torch's CPU cast) and the f32
accumulation of the FP8 matrix cores.
"""
import numpy as np
import pytest
import torch

import oracle as O
import vsg
from vsg import datagen as G
from vsg._lib import VSG_EUNSUPPORTED

pytestmark = pytest.mark.gpu


def ints(n, dim, seed):
    """Integers in [-8, 8]: l2sq sums <= dim * 256, dots <= dim * 64 -- exact f32 integers."""
    return np.random.default_rng(seed).integers(-8, 9, (n, dim)).astype(np.float32)


def e4m3(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.float8_e4m3fn).float().numpy()


def unit(a):
    """a / |a| in f32 with |a|^2 summed in the prepare kernel's order (64 lane sums of stride
    64 by fused multiply-add, then the xor butterfly): another order moves a quotient by an
    ulp now and then, and one that sat on an E4M3 tie then rounds the other way."""
    s = np.zeros((len(a), 64), np.float32)
    for j in range(0, a.shape[1], 64):
        blk = a[:, j:j + 64].astype(np.float64)
        s = (blk * blk + s).astype(np.float32)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, np.arange(64) ^ o]
    return a / np.sqrt(s[:, :1])


def answers(idx, q, k, field="exact_mfma_queries"):
    before = idx.stats()[field]
    m = idx.exact_search(q, k)
    return (m.keys, m.distances, m.counts), idx.stats()[field] - before


def same(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def new(dim, metric):
    return vsg.Index(dim, metric, "f8", exact_only=True)


@pytest.mark.parametrize("metric,dim,n,nq,k,cores", [
    ("l2sq", 256, 3001, 33, 10, True),   # two stages, ragged row tile, the 64-query tile
    ("ip", 192, 5000, 200, 16, True),    # one and a half stages, two query tiles, full k
    ("l2sq", 64, 130, 40, 7, True),      # a half stage only, fewer rows than a tile
    ("ip", 128, 1000, 257, 1, True),     # a last query tile holding one query
    ("l2sq", 128, 700, 31, 10, False),   # VALU: batch below 32
    ("ip", 72, 700, 40, 10, False),      # VALU: no whole 64-element groups
    ("l2sq", 128, 700, 40, 17, False),   # VALU: k above 16
])
def test_exact_search_bitexact_integer(metric, dim, n, nq, k, cores, monkeypatch):
    x, q = ints(n, dim, 81), ints(nq, dim, 82)
    keys = np.arange(n, dtype=np.uint64) * 3 + 11
    removed = np.zeros(n, np.uint8)
    removed[::7] = 1
    idx = new(dim, metric)
    idx.add(keys, x)
    idx.remove(keys[::7])
    ref = O.exact_search(metric, x, q, k, keys=keys, removed=removed)
    for env in ("1", "0"):
        monkeypatch.setenv("VSG_EXACT_MFMA", env)
        got, moved = answers(idx, q, k)
        assert moved == (nq if cores and env == "1" else 0)
        same(got, ref)


def test_rounding_of_edge_values():
    """Saturation (torch's cast gives NaN beyond 464 instead), subnormals, a tie."""
    row = np.array([449, 1e9, -1e9, 2.0 ** -9, 2.0 ** -11, 0, 17], np.float32)
    idx = new(7, "ip")
    idx.add(np.arange(2), np.stack([row, -row]))
    got = idx.export()["vectors"]
    want = np.array([448, 448, -448, 2.0 ** -9, 0, 0, 16], np.float32)
    np.testing.assert_array_equal(got, np.stack([want, -want]))


@pytest.mark.parametrize("metric,dim", [("ip", 256), ("l2sq", 768), ("cos", 768)])
def test_float_rows_and_distances_vs_float64(metric, dim):
    """The stored rows are torch's E4M3 cast of the prepared rows; distances against float64
    over the exported rows and the queries rounded the same way, at the bar of
    test_f16_mfma_float_vs_float64 (E4M3 x E4M3 products are exact in f32: only the f32
    accumulation is in it)."""
    n, nq, k = 4000, 150, 10
    bs, qs, ms = G.config_seeds(4)
    x, q = G.clustered(n, dim, bs, ms), G.clustered(nq, dim, qs, ms)
    assert np.abs(x).max() <= 448 and np.abs(q).max() <= 448  # in range: torch does not saturate
    idx = new(dim, metric)
    idx.add(np.arange(n), x)
    stored = idx.export()["vectors"]
    np.testing.assert_array_equal(stored, e4m3(unit(x) if metric == "cos" else x))
    xs = stored.astype(np.float64)
    qr = e4m3(unit(q) if metric == "cos" else q).astype(np.float64)
    if metric == "l2sq":
        ref = (xs * xs).sum(1)[None, :] + (qr * qr).sum(1)[:, None] - 2.0 * qr @ xs.T
    else:
        ref = 1.0 - qr @ xs.T
    order = np.argsort(ref, axis=1, kind="stable")
    rd = np.take_along_axis(ref, order, axis=1)
    (keys, dist, _), moved = answers(idx, q, k)
    assert moved == nq
    err = np.abs(dist - rd[:, :k]) / np.maximum(1.0, np.abs(rd[:, :k]))
    print(f"{metric}-{dim}: max relative distance error {err.max():.3e}")
    assert err.max() < 1e-4
    for i in range(nq):
        if set(keys[i].tolist()) != set(order[i, :k].tolist()):
            assert rd[i, k] - rd[i, k - 1] < 1e-4


def test_life_cycle_and_contract(tmp_path):
    metric, dim, n = "l2sq", 128, 3000
    x, q = ints(n, dim, 91), ints(40, dim, 92)
    keys = np.arange(n, dtype=np.uint64) * 3 + 11
    a, b = new(dim, metric), new(dim, metric)
    a.add(keys, x)
    b.add(keys[:1000], x[:1000])  # ends inside a row tile
    b.add(keys[1000:], x[1000:])
    a.save(tmp_path / "a.vsg")
    assert vsg.file_info(tmp_path / "a.vsg")["quantization"] == "f8"
    loaded, imported = vsg.Index.load(tmp_path / "a.vsg"), new(dim, metric)
    assert loaded.quantization == "f8"
    g = a.export()
    imported.import_graph(g)
    same([imported.export()[f] for f in ("vectors", "keys", "removed")], [g[f] for f in ("vectors", "keys", "removed")])
    want = answers(a, q, 10)[0]
    same(want, O.exact_search(metric, x, q, 10, keys=keys))
    for other in (b, loaded, imported):
        same(answers(other, q, 10)[0], want)
    sh = vsg.ShardedIndex(dim, metric, "f8", devices=[0, 0], exact_only=True)
    sh.add(keys, x)
    m = sh.exact_search(q, 10)
    same((m.keys, m.distances), want[:2])
    with pytest.raises(vsg.VsgError) as e:
        vsg.Index(64, "l2sq", "f8")
    assert e.value.code == VSG_EUNSUPPORTED and "EXACT_ONLY" in str(e.value)
    with pytest.raises(vsg.VsgError) as e:
        a.search(q, 10)
    assert e.value.code == VSG_EUNSUPPORTED
