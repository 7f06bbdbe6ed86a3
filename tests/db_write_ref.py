"""The reference answer of lsm_db_write, stated twice.

1. A literal restatement of go-lsm's write path: memtable.Manager.Insert /
   Delete (memtable/manager.go:40-106) with CanInsert, promoteLocked and
   MemTable.Delete's conditional (key, nil) record, over memtable_ref.py's
   SkipList and MemTable with sizeInBytes (memtable.go:68-121) added.
2. The closed form the GPU is checked against ("The
   write side"): rotation by running est sums, the extra record by "an earlier
   op of the log current before the Delete has the key".

tests/test_db_write_ref.py pins the second to the first.  An op is
(PUT, key, value) or (DELETE, key, ignored); a log is a list of (key, value)
records, value None being Go's nil (encoded as an empty value).
"""
import memtable_ref as mref

PUT, DELETE = 0, 1
TOMBSTONE = mref.TOMBSTONE
MAX_MEMTABLE_SIZE = 2 << 20  # maxMemoryTableSize


def est(key, value):
    """KeyValuePair.EstimateSize (kv.go:118-121)."""
    return 16 + len(key) + len(value)


# ---- 1. the literal Manager ---------------------------------------------------------

class SizedMemTable(mref.MemTable):
    """MemTable with sizeInBytes: Insert adds the pair's estimate
    (memtable.go:68-78), Delete adds nothing (memtable.go:84-96)."""

    def __init__(self, seed=0, size=0, nodes=()):
        super().__init__(seed)
        self.size = size
        for key, value in nodes:  # a memtable that already holds nodes (their records are not ours)
            self.entries.add(key, value)

    def can_insert(self, key, value, mem_max):  # memtable.go:112-121
        return self.size + est(key, value) <= mem_max

    def insert(self, key, value):
        super().insert(key, value)
        self.size += est(key, value)


class Manager:
    """memtable.Manager: Mem, and the promoted memtables oldest first (the
    eviction of the 11th is the binding's)."""

    def __init__(self, mem_size0=0, mem_max=MAX_MEMTABLE_SIZE, nodes=(), seed=0):
        self.mem_max = mem_max
        self.seed = seed
        self.mem = SizedMemTable(seed, mem_size0, nodes)
        self.imems = []

    def promote(self):  # promoteLocked
        self.imems.append(self.mem)
        self.seed += 1
        self.mem = SizedMemTable(self.seed)

    def insert(self, key, value):  # manager.go:40-59
        if not self.mem.can_insert(key, value, self.mem_max):
            self.promote()
        self.mem.insert(key, value)

    def delete(self, key):  # manager.go:76-106
        self.mem.delete(key)  # on the memtable current before any promotion
        self.insert(key, TOMBSTONE)

    def apply(self, ops):
        for kind, key, value in ops:
            if kind == PUT:
                self.insert(key, value)
            else:
                self.delete(key)
        return self

    def logs(self):
        return [m.wal for m in self.imems] + [self.mem.wal]


def manager_write(ops, mem_size0=0, mem_max=MAX_MEMTABLE_SIZE, nodes=()):
    """-> (logs, final sizeInBytes) by the literal Manager."""
    m = Manager(mem_size0, mem_max, nodes).apply(ops)
    return m.logs(), m.mem.size


# ---- 2. the closed form ---------------------------------------------------------------

class Written:
    """The closed form's answer: per log its records, the first op of each
    log (log_start, nlog + 1 entries), per op the (log, record index) of its
    main record, and the final size."""

    def __init__(self, logs, log_start, main, size):
        self.logs, self.log_start, self.main, self.size = logs, log_start, main, size

    @property
    def nlog(self):
        return len(self.logs)

    def log_bytes(self):
        return [mref.wal_bytes(lg) for lg in self.logs]

    def rec_base(self):
        out = [0]
        for lg in self.logs:
            out.append(out[-1] + len(lg))
        return out


def main_pair(op):
    kind, key, value = op
    return (key, value) if kind == PUT else (key, TOMBSTONE)


def write(ops, mem_size0=0, mem_max=MAX_MEMTABLE_SIZE, nodes=()):
    """The closed form.  nodes: the keys of the current memtable's nodes."""
    node_keys = {bytes(k) for k in nodes}
    logs, log_start, main = [[]], [0], []
    keys_in = [set()]  # per log, the keys of its ops so far
    size = mem_size0
    for i, op in enumerate(ops):
        key, value = main_pair(op)
        e = est(key, value)
        before = len(logs) - 1  # L(i): the log current before op i
        if size + e > mem_max:
            logs.append([])
            keys_in.append(set())
            log_start.append(i)
            size = 0
        if op[0] == DELETE and (key in keys_in[before] or (before == 0 and key in node_keys)):
            logs[before].append((key, None))
        main.append((len(logs) - 1, len(logs[-1])))
        logs[-1].append((key, value))
        keys_in[-1].add(key)
        size += e
    log_start.append(len(ops))
    return Written(logs, log_start, main, size)


def max_logs(n, key_bytes, val_bytes, mem_size0, mem_max):
    """lsm_db_write_max_logs: two consecutive logs hold more than mem_max
    between them, so floor(T / (mem_max + 1)) pairs; T bounds mem_size0 + the
    est sum from the CSR totals (a Delete's value counts 13 whatever it holds)."""
    if n == 0:
        return 1
    total = mem_size0 + 29 * n + key_bytes + val_bytes
    return min(2 * (total // (mem_max + 1)) + 2, n + 1)


def dict_model(ops, nodes=()):
    """What Manager.Search answers after the ops: key -> value (TOMBSTONE for a
    deleted key); the newest record of a key wins across the logs."""
    out = dict(nodes)
    for op in ops:
        key, value = main_pair(op)
        out[key] = value
    return out
