"""The reference answer of lsm_memtable_search and lsm_db_get, stated twice.

1. A literal restatement of go-lsm's read path over the skiplist of
   memtable_ref.py: SkipList.Search (memtable/skiplist/skiplist.go:60-79),
   Manager.Search (memtable/manager.go:61-74), Manager.Delete with its
   promotion of a full memtable (manager.go:76-106), Manager.Recover's order
   (manager.go:140-180) and database.Get (database/database.go:24-40).
2. The short form the GPU is checked against: per log a dict of last
   positions, walked newest first.

tests/test_memtable_search_ref.py pins the second to the first.  Values are
bytes; None is Go's nil.  Logs and memtables are listed OLDEST FIRST: the last
one is Mem, the others are IMems in that order.
"""
from memtable_ref import TOMBSTONE, MemTable, is_deleted

MISS, VALUE, DELETED = 0, 1, 2             # enum lsm_mem_result
EXACT, TOMBSTONE_HIDES = 0, 1              # enum lsm_db_get_mode
SRC_NONE, SRC_MEMTABLE, SRC_SSTABLE = -1, 0, 1
MAX_IMEMS = 10                             # manager.go: Recover keeps the last 10 IMems


# ---- 1. the literal restatement ------------------------------------------------

def skiplist_search(sl, key):
    """SkipList.Search, line for line -> (value, ok)."""
    curr = sl.head
    for i in range(sl.level - 1, -1, -1):
        while curr.forward[i] is not None and curr.forward[i].key < key:
            curr = curr.forward[i]
    curr = curr.forward[0]
    if curr is None or curr.key != key:
        return None, False
    if is_deleted(curr.value):
        return None, True
    return curr.value, True


class Manager:
    """memtable.Manager: Mem and IMems (oldest first), each a MemTable of
    memtable_ref.py (a skiplist and the WAL it appends to)."""

    def __init__(self, seed=0):
        self.seed = seed
        self.mem = MemTable(seed)
        self.imems = []

    def tables(self):
        """Every memtable, oldest first (the order of their WAL ids)."""
        return self.imems + [self.mem]

    def promote(self):  # promoteLocked: Mem becomes the last IMem
        self.imems.append(self.mem)
        self.seed += 1
        self.mem = MemTable(self.seed)

    def insert(self, key, value, full=False):  # Manager.Insert; full: CanInsert said no
        if full:
            self.promote()
        self.mem.insert(key, value)

    def delete(self, key, full=False):  # manager.go:76-106
        self.mem.delete(key)
        if full:
            self.promote()
        self.mem.insert(key, TOMBSTONE)

    def search(self, key):
        """Manager.Search, line for line -> value."""
        value, ok = skiplist_search(self.mem.entries, key)
        if ok:
            return value
        for i in range(len(self.imems) - 1, -1, -1):
            value, ok = skiplist_search(self.imems[i].entries, key)
            if ok:
                return value
        return None

    def search_where(self, key):
        """Manager.Search's walk with what it does not return: (the memtable
        that ended the search as an index into tables(), or -1; value; ok)."""
        t = self.tables()
        for w in range(len(t) - 1, -1, -1):
            value, ok = skiplist_search(t[w].entries, key)
            if ok:
                return w, value, True
        return -1, None, False

    @classmethod
    def recover(cls, wals, seed=0):
        """Manager.Recover: the WALs by ascending id (oldest first); the last
        becomes Mem, the others IMems in that order, the last MAX_IMEMS kept.
        A nil value went through the WAL's bytes: wal.Recover delivers it as
        an empty, non-nil value."""
        m = cls(seed)
        tables = [MemTable.recover([(k, b"" if v is None else v) for k, v in w], seed + i)
                  for i, w in enumerate(wals)]
        if tables:
            m.mem = tables[-1]
            m.imems = tables[:-1][-MAX_IMEMS:]
        return m


def database_get(memtables_search, sstables_search, key):
    """database.Get, line for line -> (value, err).  sstables_search(key) ->
    (value, err) is SSTables.Search."""
    value = memtables_search(key)
    if value is not None:
        return value, None
    value, err = sstables_search(key)
    if err is not None:
        return None, err
    if value is None:
        return None, None
    return value, None


# ---- 2. the short form -----------------------------------------------------------

def last_positions(records):
    """A log's memtable: key -> the position of its last record."""
    last = {}
    for pos, (key, _) in enumerate(records):
        last[bytes(key)] = pos
    return last


def search(logs, key, tables=None):
    """lsm_memtable_search's answer for one key over logs (oldest first; each
    a list of (key, value) as replayed: nil reads back as b"") or None for a
    log without nodes -> (result, log, position in that log, value)."""
    tables = tables if tables is not None else [None if lg is None else last_positions(lg) for lg in logs]
    for w in range(len(logs) - 1, -1, -1):
        if tables[w] is None or key not in tables[w]:
            continue
        pos = tables[w][key]
        value = logs[w][pos][1]
        value = b"" if value is None else bytes(value)
        if value == TOMBSTONE:
            return DELETED, w, pos, None
        return VALUE, w, pos, value
    return MISS, -1, -1, None


def goes_on(result, mode):
    """Whether lsm_db_get searches the tables for a key with this memtable result."""
    return result == MISS or (result == DELETED and mode == EXACT)


def get(logs, sstables_search, key, mode, tables=None):
    """lsm_db_get's answer for one key -> (src, value, err): the memtable's
    value, else SSTables.Search's for the keys that go on."""
    result, _, _, value = search(logs, key, tables)
    if not goes_on(result, mode):
        return SRC_MEMTABLE, value, None
    value, err = sstables_search(key)
    if err is not None:
        return SRC_SSTABLE, None, err
    if value is None:
        return SRC_NONE, None, None
    return SRC_SSTABLE, value, None
