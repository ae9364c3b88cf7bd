"""GPU: opt-in int8 traversal + exact f32 re-rank (VSG_FLAG_I8_TRAVERSAL; the row policy
SketchI8 of csrc/sketch_device.hpp on the register search, csrc/rerank.hip).

No usearch equivalent, so the bar is stated against this repo's own f32 walk on the same
graph:
  * integer rows and queries in [-127, 127] with a +-127 element each: the row scale is 1,
    the query scale 2^-8, every term of the sketch estimate an integer below 2^24, so the
    int8 walk evaluates the f32 walk's distances and the re-ranked top-k equals the f32
    search bit for bit (keys, distances, counts) -- also with all-zero rows and an all-zero
    query (scored in f32), across appends, capacity growth, replaces and compaction, and in
    a sharded index; with removed entries the search falls back to the f32 walk;
  * float data: every returned distance is the f32 metric value of its key (numpy f64,
    the tolerances of test_gpu_rerank.py), rows ascending, and recall@10 at least the f32
    walk's minus 0.01 at matched ef (the bar of the f16 mode);
  * vsg_stats_t.search_i8_queries tells the int8 walk from its fallbacks.
"""
import functools

import numpy as np
import pytest

import oracle as O
import vsg
from vsg import _lib
from vsg import datagen as G

pytestmark = pytest.mark.gpu

MAX_REG_EF = 1024  # vsg_kernels.hpp
N, NQ = 12000, 200


@functools.lru_cache(maxsize=None)
def int_data(n, dim, seed):
    """Integers in [-127, 127], column 0 forced to +-127 (row scale 1, query scale 2^-8)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-127, 128, size=(n, dim)).astype(np.float32)
    x[:, 0] = np.where(rng.integers(0, 2, size=n) == 1, 127.0, -127.0)
    x.setflags(write=False)
    return x


def recall(found, truth, k):
    return float(np.mean([len(set(found[i][:k].tolist()) & set(truth[i][:k].tolist())) / k
                          for i in range(truth.shape[0])]))


def _same(a, b):
    np.testing.assert_array_equal(a.keys, b.keys)
    np.testing.assert_array_equal(a.distances, b.distances)
    np.testing.assert_array_equal(a.counts, b.counts)


def i8q(idx):
    return idx.stats()["search_i8_queries"]


@pytest.mark.parametrize("metric,dim", [("ip", 64), ("l2sq", 128), ("l2sq", 100), ("ip", 72)])
def test_i8_walk_equals_f32_walk_on_integer_data(metric, dim):
    x, q = int_data(N, dim, 11), int_data(NQ, dim, 12)
    idx = vsg.Index(dim, metric, "f32", 16, 96, 64, seed=3)
    idx.add(np.arange(N), x)
    for ef, k in ((10, 10), (48, 10), (200, 32)):
        c0 = i8q(idx)
        ref = idx.search(q, k, ef)
        assert i8q(idx) == c0  # mode off: the f32 walk
        sk0 = idx.stats()["search_sketch_rows"]
        idx.set_i8_traversal(True)
        got = idx.search(q, k, ef)
        idx.set_i8_traversal(False)
        assert i8q(idx) == c0 + NQ
        assert idx.stats()["search_sketch_rows"] > sk0
        _same(got, ref)


def test_i8_walk_scores_unusable_rows_and_queries_in_f32():
    dim = 128
    x = np.concatenate([int_data(N, dim, 11), np.zeros((50, dim), np.float32)])
    q = int_data(NQ, dim, 12).copy()
    q[7] = 0.0
    idx = vsg.Index(dim, "l2sq", "f32", 16, 96, 64, seed=3)
    idx.add(np.arange(len(x)), x)
    for ef, k in ((48, 10), (200, 32)):
        ref = idx.search(q, k, ef)
        c0 = i8q(idx)
        idx.set_i8_traversal(True)
        got = idx.search(q, k, ef)
        idx.set_i8_traversal(False)
        assert i8q(idx) == c0 + NQ - 1  # the all-zero query ran the f32 walk
        _same(got, ref)
    # all-zero rows were met and scored (from their f32 rows): the all-zero query is at 0 from them
    assert got.distances[7][0] == 0 and got.keys[7][0] >= N


def test_i8_walk_tracks_appends_replaces_removals_and_compaction():
    dim, nq, n = 64, 150, 12000
    x, q = int_data(n + 741, dim, 21), int_data(nq, dim, 22)
    a = vsg.Index(dim, "l2sq", "f32", 16, 64, 40, seed=5)
    b = vsg.Index(dim, "l2sq", "f32", 16, 64, 40, seed=5, i8_traversal=True)
    caps = set()
    for s in range(0, n, 4000):  # the sketch is extended after each append and rebuilt after a growth
        a.add(np.arange(s, s + 4000), x[s:s + 4000])
        b.add(np.arange(s, s + 4000), x[s:s + 4000])
        caps.add(b.capacity())
        c0 = i8q(b)
        _same(b.search(q, 10), a.search(q, 10))
        assert i8q(b) == c0 + nq
    assert len(caps) > 1, "the appends did not cross a capacity growth"
    rng = np.random.default_rng(4)
    row = n
    for batch in (1, 40, 700):  # slots re-linked in place: their sketch rows are re-converted
        keys = rng.choice(n, batch, replace=False).astype(np.uint64)
        assert (a.replace(keys, x[row:row + batch]) == 0).all()
        assert (b.replace(keys, x[row:row + batch]) == 0).all()
        row += batch
        c0 = i8q(b)
        _same(b.search(q, 10, 48), a.search(q, 10, 48))
        assert i8q(b) == c0 + nq
    gone = np.arange(0, 3000, 2)
    assert a.remove(gone) == b.remove(gone) == 1500
    c0 = i8q(b)
    got = b.search(q, 10, 64)
    _same(got, a.search(q, 10, 64))
    assert not np.isin(got.keys, gone).any()
    assert i8q(b) == c0  # removed entries: the f32 walk (filtered search)
    assert a.compact() == b.compact() == 1500  # rows move: the sketch is rebuilt
    _same(b.search(q, 10, 64), a.search(q, 10, 64))
    assert i8q(b) == c0 + nq


@pytest.mark.parametrize("metric,dim", [("cos", 768), ("ip", 256), ("l2sq", 128)])
def test_i8_walk_float_data_exact_distances_and_recall(metric, dim):
    """Measured on an MI355X (recall@10 f32 walk / int8 walk at ef 16, ef 64): see DESIGN.md
    3.5a; the bar is the f16 mode's, the f32 walk's recall minus 0.01."""
    n, nq, k = 20000, 300, 10
    bs, qs, ms = G.config_seeds(1)
    x = G.clustered(n, dim, bs, ms)
    q = G.clustered(nq, dim, qs, ms)
    if metric == "ip":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    gk, _, _ = O.exact_search(metric, x, q, k)
    idx = vsg.Index(dim, metric, "f32", 16, 128, 64, seed=9)
    idx.add(np.arange(n), x)
    for ef in (16, 64):
        ref = idx.search(q, k, ef)
        c0 = i8q(idx)
        idx.set_i8_traversal(True)
        got = idx.search(q, k, ef)
        idx.set_i8_traversal(False)
        assert i8q(idx) == c0 + nq
        assert (got.counts == k).all()
        # distances: the f32 metric value of the returned key, ascending
        xs = x[got.keys.astype(np.int64)].astype(np.float64)
        qq = q.astype(np.float64)[:, None, :]
        if metric == "l2sq":
            want = ((xs - qq) ** 2).sum(-1)
            tol = 1e-5 * np.maximum(1.0, want)
        else:
            if metric == "cos":
                xs = xs / np.linalg.norm(xs, axis=-1, keepdims=True)
                qq = qq / np.linalg.norm(qq, axis=-1, keepdims=True)
            want = 1.0 - (xs * qq).sum(-1)
            tol = 1e-5
        assert (np.abs(got.distances - want) <= tol).all()
        assert (np.diff(got.distances, axis=1) >= 0).all()
        rg, rf = recall(got.keys, gk, k), recall(ref.keys, gk, k)
        print(f"i8_traversal recall@10 {metric} {dim} ef {ef}: f32 walk {rf:.4f} int8 walk {rg:.4f}")
        assert rg >= rf - 0.01, (ef, rg, rf)


def _einval(fn):
    with pytest.raises(vsg.VsgError) as e:
        fn()
    assert e.value.code == _lib.VSG_EINVAL, e.value


def test_i8_contract(tmp_path):
    # storage, exact-only, and each order of combining with f16 traversal
    _einval(lambda: vsg.Index(32, "l2sq", "f16", i8_traversal=True))
    _einval(lambda: vsg.Index(32, "l2sq", "f16").set_i8_traversal(True))
    _einval(lambda: vsg.Index(32, "l2sq", "f32", exact_only=True, i8_traversal=True))
    _einval(lambda: vsg.Index(32, "l2sq", "f32", exact_only=True).set_i8_traversal(True))
    _einval(lambda: vsg.Index(32, "l2sq", "f32", f16_traversal=True, i8_traversal=True))
    _einval(lambda: vsg.Index(32, "l2sq", "f32", f16_traversal=True).set_i8_traversal(True))
    _einval(lambda: vsg.Index(32, "l2sq", "f32", i8_traversal=True).set_f16_traversal(True))
    both = vsg.Index(32, "l2sq", "f32")
    both.set_i8_traversal(True)
    _einval(lambda: both.set_f16_traversal(True))
    both.set_i8_traversal(False)
    both.set_f16_traversal(True)
    _einval(lambda: both.set_i8_traversal(True))
    with pytest.raises(vsg.VsgError) as e:  # no instance above 2048 dimensions
        vsg.Index(2049, "l2sq", "f32", i8_traversal=True)
    assert e.value.code == _lib.VSG_EUNSUPPORTED and "2048" in str(e.value)

    dim = 64
    x, q = int_data(N, dim, 31), int_data(NQ, dim, 32)
    idx = vsg.Index(dim, "ip", "f32", 16, 96, 64, seed=3)
    idx.add(np.arange(N), x)
    ref = idx.search(q, 10, 48)
    idx.set_i8_traversal(True)
    _same(idx.search(q, 10, 48), ref)
    # the prefilter's switch does not take the sketch from under the int8 walk
    idx.set_prefilter(False)
    c0 = i8q(idx)
    _same(idx.search(q, 10, 48), ref)
    assert i8q(idx) == c0 + NQ
    # large ef is an error, as in the f16 mode
    with pytest.raises(vsg.VsgError) as e:
        idx.search(q, 10, MAX_REG_EF + 1)
    assert e.value.code == _lib.VSG_EUNSUPPORTED
    got = idx.search(q, 10, MAX_REG_EF)
    idx.set_i8_traversal(False)
    _same(got, idx.search(q, 10, MAX_REG_EF))
    idx.set_i8_traversal(True)
    # save / load keeps the mode and the results
    path = tmp_path / "i8.vsg"
    idx.save(path)
    assert vsg.file_info(path)["flags"] & 8
    back = vsg.Index.load(path)
    c0 = i8q(back)
    _same(back.search(q, 10, 48), ref)
    assert i8q(back) == c0 + NQ
    _einval(lambda: back.set_f16_traversal(True))


def test_i8_sharded_index_takes_the_flag():
    dim = 64
    x, q = int_data(N, dim, 11), int_data(NQ, dim, 12)
    a = vsg.ShardedIndex(dim, "ip", "f32", 16, 96, 64, devices=[0, 0], seed=3)
    b = vsg.ShardedIndex(dim, "ip", "f32", 16, 96, 64, devices=[0, 0], seed=3, i8_traversal=True)
    a.add(np.arange(N), x)
    b.add(np.arange(N), x)
    ra, rb = a.search(q, 10, 48), b.search(q, 10, 48)
    np.testing.assert_array_equal(rb.keys, ra.keys)
    assert a.stats()["search_i8_queries"] == 0
    assert b.stats()["search_i8_queries"] == 2 * NQ  # every shard walks every query
