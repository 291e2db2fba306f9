"""GPU parity of the narrow locate's LDS staging (k_locate_t's prologue,
comdb2_amd/csrc/hsc_narrow.hip) at the boundaries of its register slots: the
tiles' first codes and the packed bucket table are loaded as 16-byte pieces,
1024 threads x 2 (first codes) and x 1 (table), a staged directory as 16-byte
pieces x 3.

Every case is one index of distinct int64 keys KEY0 + KEY_STEP i ingested as
device rows (hsc_window_ingest_device) on the 8-byte-row tile pipeline
(LAYOUT_NARROW_TILES); the commit LSNs span < 2^32.  A window of `ntiles`
tiles has ntiles - 1 full 4096-row tiles and a partial last one.  One range per
read set, so every range's own verdict is compared; expected verdicts are the
CPU sort-join's (oracle/sortjoin.c) over the same rows.

  3 tiles      odd, everything in slot 0
  2049 tiles   slot 0 of the first codes exactly full (pieces 0 .. 1023) and
               the odd tail element, tile 2048, where slot 1 begins; 4096
               buckets, so the packed table's last piece holds the lone entry
               T[4096]
  2051 tiles   one piece (tiles 2048, 2049) in slot 1, and an odd tail element
  4096 tiles   the cap of the table mode: both first-code slots full
  4097 tiles   falls to the tile directory (level 0 stays in global memory)
  2049 tiles with PATH_TILE_DIR: the tile directory staged over two slots
"""

import numpy as np
import pytest

from comdb2_amd import formats as F
from comdb2_amd.formats import Range, ReadSets
from comdb2_amd.hsc import LAYOUT_AUTO, LAYOUT_NARROW, LAYOUT_NARROW_TILES, PATH_TILE_DIR, Validator
from comdb2_amd.workloads import int64_words

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = 4096            # rows per tile
KEY0, KEY_STEP = 1000, 7
LSN0 = (5 << 32) + 4096  # oldest commit; the span stays below 2^32
LSN_MOD = 1 << 20
PARTIAL = 777          # rows of the last tile


def window_rows(ntiles):
    """(keys int64[n], lsn uint64[n]): keys ascending, distinct; a row's commit
    LSN is a fixed scramble of its index, so neighbouring rows differ widely
    and every tile holds old and new rows."""
    n = (ntiles - 1) * TILE + PARTIAL
    i = np.arange(n, dtype=np.uint64)
    keys = (KEY0 + KEY_STEP * i).astype(np.int64)
    lsn = np.uint64(LSN0) + (i * np.uint64(2654435761) + (i >> np.uint64(12)) * np.uint64(40503)) % np.uint64(LSN_MOD)
    return keys, lsn


def chosen_tiles(ntiles):
    """The first four and the last four tiles, and tiles 2046-2050 (where a
    16-byte piece or a thread's slot of the staged first codes begins)."""
    t = set(range(0, 4)) | set(range(ntiles - 4, ntiles)) | set(range(2046, 2051))
    return sorted(x for x in t if 0 <= x < ntiles)


def ranges_for(ntiles, keys, seed, n_random=2000):
    """[(lo, hi)] as the module docstring lists them."""
    rng = np.random.default_rng(seed)
    first = lambda t: int(keys[t * TILE])
    last_key = int(keys[-1])
    out = []
    for t in chosen_tiles(ntiles):
        f = first(t)
        for e in (f - 1, f, f + 1):
            for w in (0, 1, KEY_STEP, 5 * KEY_STEP, 40 * KEY_STEP):
                out.append((e - w, e))   # ends at the tile's first key (+- 1)
                out.append((e, e + w))   # starts there
            out.append((e - TILE * KEY_STEP, e))      # a whole tile's worth before it
            out.append((e, e + 2 * TILE * KEY_STEP))  # two after it
    # several whole tiles
    for _ in range(200):
        a = int(rng.integers(0, ntiles))
        b = min(ntiles - 1, a + int(rng.integers(1, 12)))
        lo = first(a) + int(rng.integers(-3, 4))
        hi = first(b) + int(rng.integers(-3, TILE * KEY_STEP))
        out.append((lo, hi))
    # past the largest key: ending there, starting there, wholly past it, the whole window
    out += [(last_key - 100 * KEY_STEP, last_key + 5000), (last_key, last_key + 1),
            (last_key + 1, last_key + 10_000), (KEY0 - 50, last_key + 50), (0, KEY0 - 1)]
    # a random remainder: narrow ranges anywhere
    for _ in range(n_random):
        a = int(rng.integers(KEY0 - 100, last_key + 100))
        out.append((a, a + int(rng.integers(0, 60 * KEY_STEP))))
    return out


def snapshots_for(keys, lsn, ranges, seed):
    """A snapshot per range: the newest commit among the range's rows (not a
    conflict) or the LSN before it (a conflict), half each; a range without
    rows gets a snapshot in the middle of the span."""
    rng = np.random.default_rng(seed)
    b = np.asarray(ranges, dtype=np.int64)
    pa = np.searchsorted(keys, b[:, 0], side="left")
    pb = np.searchsorted(keys, b[:, 1], side="right")
    snaps = np.empty(len(ranges), dtype=np.uint64)
    for k in range(len(ranges)):
        if pa[k] < pb[k]:
            snaps[k] = int(lsn[pa[k]:pb[k]].max()) - int(rng.integers(0, 2))
        else:
            snaps[k] = LSN0 + LSN_MOD // 2
    return snaps


_want = {}  # ntiles -> (ReadSets, expected verdicts != 0): one sort-join per window, shared by its cases


def expected(v, oracle_mod, ntiles, keys, words, lsn):
    if ntiles not in _want:
        ranges = ranges_for(ntiles, keys, seed=ntiles)
        snaps = snapshots_for(keys, lsn, ranges, seed=ntiles + 1)
        sets = [[Range("t1", 0, F.enc_int64(a), F.enc_int64(b))] for a, b in ranges]
        rs = ReadSets.from_lists(sets, [int(s) for s in snaps], tbnames=["t1"])
        sj = oracle_mod.SortJoin(np.zeros(len(lsn), np.uint32), words, lsn, 1)
        want, _ = sj.probe(v.marshal(rs), v.table_max(), nthreads=8)
        sj.close()
        _want[ntiles] = (rs, want != 0)
    return _want[ntiles]


@pytest.fixture(scope="module")
def fresh_validator():
    v = Validator(0)
    assert v.register_group("t1", 0, 9) == 0
    yield v
    v.close()


@pytest.mark.parametrize("ntiles,paths", [(3, 0), (2049, 0), (2051, 0), (4096, 0), (4097, 0),
                                          (2049, PATH_TILE_DIR)])
def test_staging_slot_boundaries(fresh_validator, oracle_mod, ntiles, paths):
    v = fresh_validator
    keys, lsn = window_rows(ntiles)
    assert int(lsn.max()) - int(lsn.min()) < 1 << 32
    words = int64_words(keys)
    dev = torch.device("cuda", 0)
    tg = torch.zeros(len(keys), dtype=torch.int32, device=dev)
    tw = torch.from_numpy(words.reshape(-1).view(np.int64)).to(dev)
    tl = torch.from_numpy(lsn.view(np.int64)).to(dev)
    try:
        v.set_paths(paths)
        v.set_layout(LAYOUT_NARROW_TILES)
        v.ingest_device(len(keys), words.shape[0], tg.data_ptr(), tw.data_ptr(), tl.data_ptr(),
                        int(lsn.max()) + 1)
        torch.cuda.synchronize()
        assert v.layout == LAYOUT_NARROW
        rs, want = expected(v, oracle_mod, ntiles, keys, words, lsn)
        got = v.check_readsets(rs) != 0
    finally:
        v.set_paths(0)
        v.set_layout(LAYOUT_AUTO)
    np.testing.assert_array_equal(got, want)
    assert 0 < int(want.sum()) < len(want)
