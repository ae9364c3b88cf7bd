"""GPU: the integer sketch pass of the prefiltered register search (csrc/sketch.hpp,
sketch_device.hpp).  Every case searches one small index with the prefilter forced on and
forced off: keys, distances, counts and the search_distances counter must be equal bit for
bit -- for every prefiltered row shape (256-d = 1 KiB rows, 264, 512, 768, 1024, 1536,
2048-d = 8 KiB rows), both sides of every register-row class (ef 36, 64 | 65, 192 | 193),
cos and ip with un-normalised rows, and queries whose quantisation is at its limits
(all-zero, scaled by 1e20 / 1e-20, one-hot, integer-valued with exact ties).  The persistent
grid's fraction forced to 1.0 and to 0.05 in child processes gives the default's results."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vsg

pytestmark = pytest.mark.gpu

K = 10
N = 3000
NQ = 96
DIMS = [256, 264, 512, 768, 1024, 1536, 2048]  # 512 and 1024: the two row shapes between
EFS = [36, 64, 65, 192, 193]
PKG = os.path.dirname(os.path.dirname(os.path.abspath(vsg.__file__)))


def _search(idx, q, ef, k=K):
    nq = q.shape[0]
    before = idx.stats()["search_distances"]
    oc = torch.empty(nq, dtype=torch.int32, device="cuda")
    ok, od = idx.search_device(q, k, ef, out_counts=oc)
    torch.cuda.synchronize()
    return ok.clone(), od.clone(), oc.clone(), idx.stats()["search_distances"] - before


def _on_off(idx, q, ef, what=""):
    """on == off bit for bit; returns (sketch rows, f32 rows at level 0) of the on search"""
    idx.set_prefilter(True)
    s0 = idx.stats()
    on = _search(idx, q, ef)
    s1 = idx.stats()
    idx.set_prefilter(False)
    off = _search(idx, q, ef)
    assert torch.equal(on[0], off[0]), f"keys differ {what}"
    assert torch.equal(on[1].view(torch.int32), off[1].view(torch.int32)), f"distances differ {what}"
    assert torch.equal(on[2], off[2]), f"counts differ {what}"
    assert on[3] == off[3], f"search_distances differ {what}: {on[3]} != {off[3]}"
    return s1["search_sketch_rows"] - s0["search_sketch_rows"], s1["search_exact_rows"] - s0["search_exact_rows"]


def _rows(dim, metric):
    x = vsg.datagen_device("clustered", N, dim, 0x5EED0010 + dim, 0x5EED2010)
    if metric == "ip":
        # un-normalised: norms over 100x, a block of integer-valued rows, 50 duplicates
        g = torch.Generator(device="cpu").manual_seed(dim)
        norms = torch.exp(torch.empty(N, 1).uniform_(float(np.log(0.1)), float(np.log(10.0)), generator=g)).cuda()
        x = x * norms
        x[2000:] = torch.round(x[2000:] * (20.0 / norms[2000:]))
        x[2500:2550] = x[2499]
    return x.contiguous()


_cache = {}


@pytest.fixture(scope="module")
def index_of():
    """one index per (dim, metric), built on first use"""
    def get(dim, metric):
        if (dim, metric) not in _cache:
            x = _rows(dim, metric)
            idx = vsg.Index(dim, metric, "f32", 16, 64, 36, seed=11)
            idx.add_device(np.arange(N), x)
            torch.cuda.synchronize()
            q = vsg.datagen_device("clustered", NQ, dim, 0x5EED1010 + dim, 0x5EED2010)
            _cache[(dim, metric)] = (idx, x, q)
        return _cache[(dim, metric)]
    yield get
    for idx, _, _ in _cache.values():
        idx.close()
    _cache.clear()


@pytest.mark.parametrize("metric", ["cos", "ip"])
@pytest.mark.parametrize("dim", DIMS)
def test_on_equals_off(index_of, dim, metric):
    idx, _, q = index_of(dim, metric)
    for ef in EFS:
        nsk, _ = _on_off(idx, q, ef, what=f"dim {dim} {metric} ef {ef}")
        assert nsk > 0, f"dim {dim} {metric} ef {ef}: the prefilter never ran"


def _edge_queries(x, q, dim):
    """all-zero, 1e20 / 1e-20 scaled, one-hot, integer-valued (exact ties on the integer rows)"""
    e = []
    e.append(torch.zeros(4, dim, device="cuda"))
    e.append(q[:16] * 1e20)
    e.append(q[16:32] * 1e-20)
    hot = torch.zeros(8, dim, device="cuda")
    for i, j in enumerate([0, 1, 15, 16, dim // 2, dim - 2, dim - 1, 17]):
        hot[i, j] = -1.0 if i % 2 else 1.0
    e.append(hot)
    e.append(torch.round(q[32:64] * 30.0))
    e.append(torch.round(x[2495:2505] * 3.0))   # multiples of rows, the duplicated one among them
    e.append(torch.full((2, dim), 0.0361, device="cuda") * torch.tensor([[1.0], [-1.0]], device="cuda"))
    return torch.cat(e).contiguous()


@pytest.mark.parametrize("metric", ["cos", "ip"])
@pytest.mark.parametrize("dim", DIMS)
def test_edge_queries_on_equals_off(index_of, dim, metric):
    idx, x, q = index_of(dim, metric)
    eq = _edge_queries(x, q, dim)
    for ef in (36, 65):
        _on_off(idx, eq, ef, what=f"edge queries dim {dim} {metric} ef {ef}")


def test_filter_bites(index_of):
    idx, _, _ = index_of(768, "cos")
    q = vsg.datagen_device("clustered", 2048, 768, 0x5EED1011, 0x5EED2010)
    nsk, nex = _on_off(idx, q, 36, what="2,048 queries")
    print(f"sketch rows {nsk}, f32 rows at level 0 {nex}: {nex / max(1, nsk):.3f}")
    assert nsk > 0
    assert nex < nsk


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import vsg
idx = vsg.Index.load(sys.argv[2])
idx.set_prefilter(True)
q = torch.from_numpy(np.load(sys.argv[3])).cuda()
k, d = idx.search_device(q, 10, 36)
torch.cuda.synchronize()
assert idx.stats()["search_sketch_rows"] > 0
np.savez(sys.argv[4], keys=k.cpu().numpy(), dist=d.cpu().numpy().view(np.int32))
"""


def test_forced_persistent_fraction(index_of, tmp_path):
    """VSG_SEARCH_PERSIST_FRAC is read once per process: 1.0 and 0.05 in fresh children."""
    idx, _, _ = index_of(768, "cos")
    q = vsg.datagen_device("clustered", 2048, 768, 0x5EED1012, 0x5EED2010)
    idx.set_prefilter(True)
    rk, rd = idx.search_device(q, K, 36)
    torch.cuda.synchronize()
    path, qpath = str(tmp_path / "pf.vsg"), str(tmp_path / "q.npy")
    idx.save(path)
    np.save(qpath, q.cpu().numpy())
    children = []
    for frac in ("1.0", "0.05"):
        env = dict(os.environ, VSG_SEARCH_PERSIST_FRAC=frac)
        out = str(tmp_path / f"out_{frac}.npz")
        children.append((frac, out, subprocess.Popen([sys.executable, "-c", _CHILD, PKG, path, qpath, out], env=env,
                                                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for frac, out, p in children:
        log, _ = p.communicate(timeout=300)
        assert p.returncode == 0, f"fraction {frac}: {log[-2000:]}"
        z = np.load(out)
        assert np.array_equal(z["keys"], rk.cpu().numpy()), f"keys differ at fraction {frac}"
        assert np.array_equal(z["dist"], rd.cpu().numpy().view(np.int32)), f"distances differ at fraction {frac}"
