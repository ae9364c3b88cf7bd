"""GPU: one life cycle for the three derived copies of the rows that share one upkeep
(csrc/vsg_index.cpp RowCopy / row_copy_ensure): the f16 traversal copy, the int8 sketch
of the prefilter and the K-tiled MFMA copy of exact-only indexes.  After every change of
the rows -- add, capacity growth, an add that ends inside a 256-row tile, removals,
re-adds into freed slots, compaction, the copy switched off and on -- the search that
reads the copy returns the keys, distances and counts of the same index searched with
the copy disabled, bit for bit; the exact-only index also equals the oracle.

dim 256: 1 KiB f32 rows, the smallest the prefilter takes, and whole 32-dim stages for
the K-tiled copy.  Rows are integers 0..15 under ip, so f16 holds them exactly, every
partial sum is an integer < 2^24 and equal distances are frequent."""
import numpy as np
import pytest
import torch

import oracle as O
import vsg
from vsg import datagen as G

pytestmark = pytest.mark.gpu

DIM, K, EF = 256, 10, 32
N0, N1 = 700, 1000  # 1000 rows end inside the fourth 256-row tile
REMOVED = np.arange(0, N1, 7)
READDED = REMOVED[:50]


@pytest.fixture(scope="module")
def rows():
    x = np.floor(G.uint8_valued(N1, DIM, 0x5EED0401) / 16).astype(np.float32)
    q = np.floor(G.uint8_valued(64, DIM, 0x5EED0402) / 16).astype(np.float32)
    return x, q


def _search(idx, qt, exact):
    oc = torch.empty(qt.shape[0], dtype=torch.int32, device="cuda")
    ok, od = idx.search_device(qt, K, EF, out_counts=oc, exact=exact)
    torch.cuda.synchronize()
    return ok.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy()


def _assert_same(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=f"keys differ {what}")
    # bit for bit: compare the words (-0 != +0)
    np.testing.assert_array_equal(a[1].view(np.int32), b[1].view(np.int32), err_msg=f"distances differ {what}")
    np.testing.assert_array_equal(a[2], b[2], err_msg=f"counts differ {what}")


class _F16:
    exact, nq, reuse = False, 64, True

    def make(self):
        idx = vsg.Index(DIM, "ip", "f32", 16, 64, EF, seed=4)
        idx.set_f16_traversal(True)
        return idx

    def on(self, idx, mp):
        idx.set_f16_traversal(True)

    def off(self, idx, mp):
        idx.set_f16_traversal(False)  # frees the copy


class _Sketch:
    exact, nq, reuse = False, 64, True

    def make(self):
        idx = vsg.Index(DIM, "ip", "f32", 16, 64, EF, seed=4)
        idx.set_prefilter(True)
        return idx

    def on(self, idx, mp):
        idx.set_prefilter(True)

    def off(self, idx, mp):
        idx.set_prefilter(False)  # frees the copy


class _Ktile:
    # 40 queries: the MFMA search (>= 32 queries), the 256 x 64 tile.  An exact-only index
    # never re-links freed slots (reuse_on), so the re-add step does not apply
    exact, nq, reuse = True, 40, False

    def make(self):
        return vsg.Index(DIM, "ip", "f32", exact_only=True)

    def on(self, idx, mp):
        mp.delenv("VSG_EXACT_KTILE", raising=False)

    def off(self, idx, mp):
        mp.setenv("VSG_EXACT_KTILE", "0")  # the row-major loads; the copy stays


@pytest.mark.parametrize("copy", [_F16(), _Sketch(), _Ktile()], ids=["f16", "sketch", "ktile"])
def test_copy_tracks_the_rows_through_a_life_cycle(copy, rows, monkeypatch):
    x, q = rows
    qt = torch.from_numpy(q[:copy.nq]).cuda()
    keys = np.arange(N1, dtype=np.uint64) * 3 + 1
    removed = np.zeros(N1, np.uint8)
    idx = copy.make()

    def check(what):
        copy.on(idx, monkeypatch)
        s0 = idx.stats()["search_sketch_rows"]
        on = _search(idx, qt, copy.exact)
        if isinstance(copy, _Sketch) and idx.free_slots().size == 0:
            # the prefilter applies to indexes without removed entries: there the search read the sketch
            assert idx.stats()["search_sketch_rows"] > s0, f"the sketch was not read {what}"
        copy.off(idx, monkeypatch)
        off = _search(idx, qt, copy.exact)
        _assert_same(on, off, what)
        if copy.exact:
            ok, od, oc = O.exact_search("ip", x[idx_rows], q[:copy.nq], K, keys=keys[idx_rows],
                                        removed=removed[idx_rows])
            _assert_same(on, (ok.astype(np.int64), od, oc.astype(np.int32)), what + " (oracle)")
        copy.on(idx, monkeypatch)
        _search(idx, qt, copy.exact)  # the next step starts from a current copy

    idx.add(keys[:N0], x[:N0])
    idx_rows = np.arange(N0)  # rows of x in the index, in slot order (exact-only: nothing is re-linked)
    check("after the first add")

    idx.reserve(idx.capacity() + 1000)
    check("after a capacity growth")

    idx.add(keys[N0:], x[N0:])
    idx_rows = np.arange(N1)
    check("after an add that ends inside a tile")

    assert idx.remove(keys[REMOVED]) == len(REMOVED)
    removed[REMOVED] = 1
    check("after removals")

    if copy.reuse:
        idx.add(keys[READDED], x[READDED])  # re-links freed slots: those rows are rewritten in place
        assert idx.stats()["slots_reused"] > 0
        check("after re-adds into freed slots")

    assert idx.compact() > 0  # rows move
    if copy.exact:
        idx_rows = np.flatnonzero(removed == 0)
    check("after a compaction")

    copy.off(idx, monkeypatch)
    copy.on(idx, monkeypatch)
    check("after the copy was switched off and on")
    idx.close()
