"""lsm_pack_results restated in numpy (include/lsm_gpu.h): plain loops over the
slots, slicing host copies of the two source buffers.  Pinned against a case
written out literally in tests/test_pack_ref.py."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

SRC_NONE, SRC_MEMTABLE, SRC_SSTABLE = -1, 0, 1
DESC = np.dtype([("rec_off", "<u8"), ("key_len", "<u4"), ("val_len", "<u4")])


@dataclass
class PackedRef:
    row_start: np.ndarray            # uint64[nrow + 1]
    entry_slot: np.ndarray           # uint32[E]
    koff: Optional[np.ndarray]       # uint64[E + 1]; None when no keys are packed
    voff: np.ndarray                 # uint64[E + 1]
    keys: Optional[bytes]            # the K key bytes; None when the key arena is not written
    vals: Optional[bytes]            # the V value bytes; None when the value arena is not written
    counts: np.ndarray               # uint64[4]: {E, K, V, overflow}


def pack(wal, img, src, key, value, count, nrow, limit, key_cap=None, val_cap=None):
    """wal / img: the host copies of d_bytes / d_img (bytes-like or None for a
    NULL pointer); src / key / count: arrays or None as the C arguments; key /
    value: DESC arrays over the nrow * limit slots.  key_cap / val_cap None: that
    arena is NULL.  keys / vals of the result are None where the call writes no
    byte of that arena (a NULL arena, or overflow)."""
    assert limit > 0
    row_start, entry_slot, klen, vlen = [], [], [], []
    kparts, vparts = [], []
    for q in range(nrow):
        row_start.append(len(entry_slot))
        live = limit if count is None else min(int(count[q]), limit)
        for j in range(live):
            o = q * limit + j
            s = SRC_SSTABLE if src is None else int(src[o])
            base = wal if s == SRC_MEMTABLE else img if s == SRC_SSTABLE else None
            k = v = b""
            if base is not None:
                at, n = int(value[o]["rec_off"]) + 4, int(value[o]["val_len"])
                v = bytes(base[at:at + n])
                assert len(v) == n, "a live view must lie inside its buffer"
                if key is not None:
                    at, n = int(key[o]["rec_off"]) + 4, int(key[o]["key_len"])
                    k = bytes(base[at:at + n])
                    assert len(k) == n, "a live view must lie inside its buffer"
            entry_slot.append(o)
            klen.append(len(k))
            vlen.append(len(v))
            kparts.append(k)
            vparts.append(v)
    row_start.append(len(entry_slot))
    E = len(entry_slot)
    koff = np.concatenate([[0], np.cumsum(klen)]).astype(np.uint64)
    voff = np.concatenate([[0], np.cumsum(vlen)]).astype(np.uint64)
    K, V = int(koff[-1]), int(voff[-1])
    overflow = int((key_cap is not None and K > key_cap) or (val_cap is not None and V > val_cap))
    written = not overflow
    return PackedRef(
        row_start=np.array(row_start, np.uint64), entry_slot=np.array(entry_slot, np.uint32),
        koff=koff if key is not None else None, voff=voff,
        keys=b"".join(kparts) if (written and key_cap is not None) else None,
        vals=b"".join(vparts) if (written and val_cap is not None) else None,
        counts=np.array([E, K, V, overflow], np.uint64))
