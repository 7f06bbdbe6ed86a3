"""The reference answer of lsm_memtable_order, stated twice.

1. A literal restatement of go-lsm's memtable: SkipList.Add / Delete
   (memtable/skiplist/skiplist.go:83-150), the skiplist iterator
   (skiplist/iterator.go:27-33, 68-80), IMemTable.RangeScan
   (memtable/imemtable.go:46-53), MemTable.Insert / Delete (memtable.go:68-96)
   and Manager.Delete (memtable/manager.go:76-106) with the WAL they append to.
2. The short form the GPU is checked against: a dict by last position, sorted
   by bytes, then RangeScan's cut.

tests/test_memtable_ref.py pins the second to the first.  Values are bytes;
None is Go's nil value, which the WAL encodes as an empty value.
"""
import random
import struct

TOMBSTONE = "～DELETED～".encode()  # kv.DeletedValue (kv/kv.go:29)
ALL, RANGESCAN = 0, 1
MAX_LEVEL, P_FACTOR = 32, 0.25       # skiplist.go:19-22


def is_deleted(value):
    """KeyValuePair.IsDeleted (kv.go:40-43)."""
    return value is not None and bytes(value) == TOMBSTONE


class Node:
    def __init__(self, key, value, levels):
        self.key, self.value = key, value
        self.forward = [None] * levels


class SkipList:
    """skiplist.go, line for line; randomLevel draws from a seeded generator."""

    def __init__(self, seed=0):
        self.head = Node(b"", None, MAX_LEVEL)
        self.level = 0
        self.rng = random.Random(seed)

    def random_level(self):
        lv = 1
        while lv < MAX_LEVEL and self.rng.random() < P_FACTOR:
            lv += 1
        return lv

    def add(self, key, value):
        update = [None] * MAX_LEVEL
        curr = self.head
        for i in range(self.level - 1, -1, -1):
            while curr.forward[i] is not None and curr.forward[i].key < key:
                curr = curr.forward[i]
            update[i] = curr
        nxt = curr.forward[0]
        if nxt is not None and nxt.key == key:
            nxt.value = value
            return
        lv = self.random_level()
        if lv > self.level:
            for i in range(self.level, lv):
                update[i] = self.head
            self.level = lv
        node = Node(key, value, lv)
        for i in range(lv):
            node.forward[i] = update[i].forward[i]
            update[i].forward[i] = node

    def delete(self, key):
        update = [None] * MAX_LEVEL
        curr = self.head
        for i in range(self.level - 1, -1, -1):
            while curr.forward[i] is not None and curr.forward[i].key < key:
                curr = curr.forward[i]
            update[i] = curr
        target = curr.forward[0]
        if target is None or target.key != key:
            return False
        target.value = TOMBSTONE
        for i in range(self.level):
            if update[i].forward[i] is not target:
                break
            update[i].forward[i] = target.forward[i]
        while self.level > 1 and self.head.forward[self.level - 1] is None:
            self.level -= 1
        return True

    def nodes(self):
        """Every linked node in level-0 order."""
        out, curr = [], self.head.forward[0]
        while curr is not None:
            out.append((curr.key, curr.value))
            curr = curr.forward[0]
        return out

    def range_scan(self):
        """RangeScan: `for iter.SeekToFirst(); iter.Valid(); iter.Next()`."""
        curr = self.head.forward[0]
        while curr is not None and is_deleted(curr.value):  # SeekToFirst
            curr = curr.forward[0]
        out = []
        while curr is not None and not is_deleted(curr.value):  # Valid
            out.append((curr.key, curr.value))
            curr = curr.forward[0]  # Next
        return out


class MemTable:
    """MemTable over a skiplist and a WAL kept as a list of (key, value)."""

    def __init__(self, seed=0):
        self.entries = SkipList(seed)
        self.wal = []

    def insert(self, key, value):  # memtable.go:68-78: the WAL first, then AddPair
        self.wal.append((key, value))
        self.entries.add(key, value)

    def delete(self, key):  # memtable.go:84-96: nil value to the WAL when the node existed
        if self.entries.delete(key):
            self.wal.append((key, None))

    def manager_delete(self, key):  # manager.go:76-106 (the memtable never fills here)
        self.delete(key)
        self.insert(key, TOMBSTONE)

    @classmethod
    def recover(cls, wal, seed=0):  # RecoverFromWAL: AddPairs of the log's records
        t = cls(seed)
        for key, value in wal:
            t.entries.add(key, value)
        return t


def wal_bytes(wal):
    """KeyValuePair.EncodeTo (kv.go:46-74) of every record; nil encodes empty."""
    out = []
    for key, value in wal:
        v = b"" if value is None else bytes(value)
        out.append(struct.pack("<I", len(key)) + key + struct.pack("<I", len(v)) + v)
    return b"".join(out)


def order(records, scan=ALL):
    """The short form.  records: the log's (key, value) in append order ->
    the positions delivered, in order: per key the last position, by key
    bytes; RANGESCAN skips the tombstones at the front and stops before the
    first one after that."""
    last = {}
    for pos, (key, _) in enumerate(records):
        last[bytes(key)] = pos
    out = [last[k] for k in sorted(last)]
    if scan == ALL:
        return out
    dead = [is_deleted(b"" if records[p][1] is None else records[p][1]) for p in out]
    i = 0
    while i < len(out) and dead[i]:
        i += 1
    j = i
    while j < len(out) and not dead[j]:
        j += 1
    return out[i:j]
