"""GPU: the int8 sketch prefilter of the register search (vsg_index_set_prefilter;
csrc/sketch.hpp, hnsw_regset.hpp beam_reg).  Every case searches one index with the
prefilter on and off: keys, distances, counts and the search_distances counter must be
equal bit for bit -- the prefilter only skips f32 rows of candidates that could not
have been admitted."""
import numpy as np
import pytest
import torch

import vsg

pytestmark = pytest.mark.gpu

K = 10


def _search(idx, q, ef, k=K, stream=None):
    """(keys, distances, counts, distance evaluations) of one device search."""
    nq = q.shape[0]
    before = idx.stats()["search_distances"]
    oc = torch.empty(nq, dtype=torch.int32, device="cuda")
    ok, od = idx.search_device(q, k, ef, out_counts=oc, stream=stream)
    torch.cuda.synchronize()
    return ok.clone(), od.clone(), oc.clone(), idx.stats()["search_distances"] - before


def _assert_same(a, b, what=""):
    assert torch.equal(a[0], b[0]), f"keys differ {what}"
    # bit for bit: compare the words (NaN-safe, -0 != +0)
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), f"distances differ {what}"
    assert torch.equal(a[2], b[2]), f"counts differ {what}"
    assert a[3] == b[3], f"search_distances differ {what}: {a[3]} != {b[3]}"


def _on_off(idx, q, ef, k=K, what=""):
    idx.set_prefilter(True)
    s0 = idx.stats()
    on = _search(idx, q, ef, k)
    s1 = idx.stats()
    idx.set_prefilter(False)
    off = _search(idx, q, ef, k)
    s2 = idx.stats()
    assert s2["search_sketch_rows"] == s1["search_sketch_rows"], "prefilter off still read sketch rows"
    _assert_same(on, off, what)
    idx.set_prefilter(True)
    return on, s1["search_sketch_rows"] - s0["search_sketch_rows"], s1["search_exact_rows"] - s0["search_exact_rows"]


@pytest.fixture(scope="module")
def clustered():
    n, dim = 20000, 768
    x = vsg.datagen_device("clustered", n, dim, 0x5EED0002, 0x5EED2002)
    q = vsg.datagen_device("clustered", 256, dim, 0x5EED1002, 0x5EED2002)
    idx = vsg.Index(dim, "cos", "f32", 16, 64, 36, seed=7)
    idx.add_device(np.arange(n), x)
    torch.cuda.synchronize()
    return idx, x, q


# both sides of every register-row class the prefilter is compiled for (2: ef <= 64,
# 4: <= 192, 8: <= 448)
@pytest.mark.parametrize("ef", [10, 36, 64, 65, 192, 193, 448])
def test_clustered_on_equals_off(clustered, ef):
    idx, _, q = clustered
    _, nsk, nex = _on_off(idx, q, ef, what=f"ef {ef}")
    assert nsk > 0


def test_engagement_counters(clustered):
    idx, _, q = clustered
    on, nsk, nex = _on_off(idx, q, 36)
    print(f"sketch rows {nsk}, f32 rows at level 0 {nex}, distance evaluations {on[3]}: "
          f"f32 rows / evaluations = {nex / on[3]:.3f}")
    assert nsk > 0
    assert 0 < nex < on[3]


@pytest.mark.parametrize("ef", [36, 128])
def test_ties_integer_rows(ef):
    # integer-valued rows under ip: many exact distance ties, candidates exactly at the bound
    n, dim = 20000, 768
    x = vsg.datagen_device("sift", n, dim, 0x5EED0004, 0x5EED2004)
    q = vsg.datagen_device("sift", 256, dim, 0x5EED1004, 0x5EED2004)
    idx = vsg.Index(dim, "ip", "f32", 16, 64, 36, seed=3)
    idx.add_device(np.arange(n), x)
    _on_off(idx, q, ef, what=f"sift ip ef {ef}")
    idx.close()


def test_unnormalised_ip_rows():
    n, dim = 8000, 768
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x *= np.exp(rng.uniform(np.log(0.1), np.log(10.0), size=(n, 1))).astype(np.float32)  # norms over 100x
    x[17] = rng.standard_normal(dim).astype(np.float32)
    x[17, 5] = 1e6  # one outlier element
    x[18] = 0.0     # all-zero row
    x[100:150] = x[99]  # 50 duplicates
    q = rng.standard_normal((256, dim)).astype(np.float32)
    q[:8] = x[[17, 18, 99, 100, 120, 149, 5, 6]]
    idx = vsg.Index(dim, "ip", "f32", 16, 64, 36, seed=5)
    idx.add(np.arange(n), x)
    qt = torch.from_numpy(q).cuda()
    for ef in (36, 100):
        _on_off(idx, qt, ef, what=f"ip ef {ef}")
    idx.close()


@pytest.mark.parametrize("dim", [1536, 264])
def test_other_row_shapes(dim):
    # 1536: another row shape; 264: 1,056-B rows whose sketch row is not whole 16-B chunks
    n = 12000
    x = vsg.datagen_device("clustered", n, dim, 0x5EED0005, 0x5EED2005)
    q = vsg.datagen_device("clustered", 256, dim, 0x5EED1005, 0x5EED2005)
    idx = vsg.Index(dim, "cos", "f32", 16, 64, 36, seed=9)
    idx.add_device(np.arange(n), x)
    for ef in (36, 100):
        _, nsk, _ = _on_off(idx, q, ef, what=f"dim {dim} ef {ef}")
        assert nsk > 0
    idx.close()


def test_sketch_upkeep(tmp_path):
    """After each change of the rows the first prefiltered search equals the plain one."""
    dim, n0 = 768, 6000
    x = vsg.datagen_device("clustered", 2 * n0 + 100, dim, 0x5EED0006, 0x5EED2006)
    q = vsg.datagen_device("clustered", 256, dim, 0x5EED1006, 0x5EED2006)
    idx = vsg.Index(dim, "cos", "f32", 16, 64, 36, seed=2)
    idx.reserve(n0 + 500)
    idx.add_device(np.arange(n0), x[:n0].contiguous())
    idx.set_prefilter(True)
    _search(idx, q, 36)  # builds the sketch

    def check(what):
        idx.set_prefilter(True)  # keeps the rows it has
        on = _search(idx, q, 36)
        sk = idx.stats()["search_sketch_rows"]
        assert sk > 0
        # off frees the sketch; the comparison search is the plain kernel
        idx.set_prefilter(False)
        off = _search(idx, q, 36)
        _assert_same(on, off, what)
        idx.set_prefilter(True)
        _search(idx, q, 36)  # rebuilt: the next step starts from a current sketch
        return on

    # incremental conversion: a second add within the capacity
    idx.add_device(np.arange(n0, n0 + 400), x[n0:n0 + 400].contiguous())
    check("after a second add")
    # capacity growth
    idx.reserve(2 * n0 + 100)
    idx.add_device(np.arange(n0 + 400, 2 * n0), x[n0 + 400:2 * n0].contiguous())
    check("after reserve growth")
    # replace of 100 keys: their rows are rewritten
    idx.replace(np.arange(100, 200), x[2 * n0:2 * n0 + 100].cpu().numpy())
    check("after replace")
    # save and load
    path = str(tmp_path / "pf.vsg")
    idx.save(path)
    idx2 = vsg.Index.load(path)
    a = _on_off(idx2, q, 36, what="loaded index")[0]
    idx.set_prefilter(False)
    b = _search(idx, q, 36)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    idx2.close()
    idx.close()


def test_opt_in_modes_unchanged(clustered):
    idx, _, q = clustered
    try:
        # multi-entry descent: the level-0 beam is seeded; on == off
        idx.set_upper_ef(16)
        _on_off(idx, q, 36, what="upper_ef 16")
        idx.set_upper_ef(0)
        # f16 traversal: the prefilter does not apply, whatever the switch says
        idx.set_f16_traversal(True)
        s0 = idx.stats()["search_sketch_rows"]
        _on_off(idx, q, 36, what="f16 traversal")
        assert idx.stats()["search_sketch_rows"] == s0
    finally:
        idx.set_f16_traversal(False)
        idx.set_upper_ef(0)
        idx.set_prefilter(True)


def test_two_streams_equal_sequential(clustered):
    idx, _, q = clustered
    idx.set_prefilter(True)
    qa = vsg.datagen_device("clustered", 2048, 768, 0x5EED1007, 0x5EED2002)
    batches = [qa[:1024].contiguous(), qa[1024:].contiguous()]
    ref = [_search(idx, b, 36) for b in batches]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for b, s in zip(batches, streams):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            k = torch.empty((1024, K), dtype=torch.int64, device="cuda")
            d = torch.empty((1024, K), dtype=torch.float32, device="cuda")
            c = torch.empty(1024, dtype=torch.int32, device="cuda")
            idx.search_device(b, K, 36, out_keys=k, out_dist=d, out_counts=c, stream=s.cuda_stream)
        outs.append((k, d, c))
    torch.cuda.synchronize()
    for (k, d, c), r in zip(outs, ref):
        assert torch.equal(k, r[0]) and torch.equal(d.view(torch.int32), r[1].view(torch.int32)) and torch.equal(c, r[2])
