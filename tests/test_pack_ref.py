"""Pins tests/pack_ref.py (the numpy restatement of lsm_pack_results the GPU
tests compare against) to a case written out literally: 3 rows of 2 slots with
counts {2, 0, 1}, both sources, one LSM_SRC_NONE entry and one empty value."""
import numpy as np

import pack_ref
from pack_ref import DESC, SRC_MEMTABLE, SRC_NONE, SRC_SSTABLE

WAL = bytes(range(100, 140))   # byte i is 100 + i
IMG = bytes(range(200, 240))   # byte i is 200 + i


def literal():
    key = np.zeros(6, DESC)
    value = np.zeros(6, DESC)
    src = np.array([SRC_MEMTABLE, SRC_SSTABLE, SRC_SSTABLE, SRC_MEMTABLE, SRC_NONE, SRC_SSTABLE], np.int32)
    key[0], value[0] = (0, 3, 2), (7, 0, 2)        # a KV record at 0: key WAL[4:7], value WAL[11:13]
    key[1], value[1] = (10, 1, 8), (20, 0, 0)      # an IDX entry: key IMG[14:15], an empty value
    key[2], value[2] = (1, 5, 8), (2, 0, 7)        # row 1 holds nothing: decoys
    key[3], value[3] = (3, 2, 4), (9, 0, 4)
    key[4], value[4] = (5, 4, 8), (6, 0, 9)        # LSM_SRC_NONE: an entry of no bytes whatever the views say
    key[5], value[5] = (8, 6, 8), (12, 0, 3)       # past row 2's count: a decoy
    count = np.array([2, 0, 1], np.uint32)
    return src, key, value, count


def test_literal_case():
    src, key, value, count = literal()
    p = pack_ref.pack(WAL, IMG, src, key, value, count, 3, 2, key_cap=4, val_cap=2)
    assert p.row_start.tolist() == [0, 2, 2, 3]
    assert p.entry_slot.tolist() == [0, 1, 4]
    assert p.koff.tolist() == [0, 3, 4, 4]
    assert p.voff.tolist() == [0, 2, 2, 2]
    assert p.keys == bytes([104, 105, 106, 214])
    assert p.vals == bytes([111, 112])
    assert p.counts.tolist() == [3, 4, 2, 0]


def test_caps_and_null_arguments():
    src, key, value, count = literal()
    # one byte short in either arena: the flag, no byte of either, everything else as before
    for caps in ((3, 2), (4, 1)):
        p = pack_ref.pack(WAL, IMG, src, key, value, count, 3, 2, key_cap=caps[0], val_cap=caps[1])
        assert p.counts.tolist() == [3, 4, 2, 1] and p.keys is None and p.vals is None
        assert p.koff.tolist() == [0, 3, 4, 4] and p.voff.tolist() == [0, 2, 2, 2]
    # the sizing call
    p = pack_ref.pack(WAL, IMG, src, key, value, count, 3, 2)
    assert p.counts.tolist() == [3, 4, 2, 0] and p.keys is None and p.vals is None
    # no keys; a NULL d_bytes turns the memtable entry into one of no bytes
    p = pack_ref.pack(None, IMG, src, None, value, count, 3, 2, val_cap=0)
    assert p.koff is None and p.voff.tolist() == [0, 0, 0, 0] and p.counts.tolist() == [3, 0, 0, 0]
    assert p.vals == b""
    # d_count NULL: every slot is live; d_src NULL: every slot reads the images
    p = pack_ref.pack(None, IMG, None, key, value, None, 3, 2, key_cap=100, val_cap=100)
    assert p.row_start.tolist() == [0, 2, 4, 6] and p.entry_slot.tolist() == list(range(6))
    assert p.koff.tolist() == [0, 3, 4, 9, 11, 15, 21]
    assert p.keys[:3] == bytes([204, 205, 206]) and p.vals[:2] == bytes([211, 212])
    # a count above limit is clamped
    p = pack_ref.pack(WAL, IMG, src, key, value, np.array([7, 0, 1], np.uint32), 3, 2, key_cap=4, val_cap=2)
    assert p.row_start.tolist() == [0, 2, 2, 3]
