"""Pins db_write_ref.write (the closed form lsm_db_write is checked against) to
the literal restatement of memtable.Manager.Insert / Delete over the restated
skiplist, on random batches, and pins the lsm_db_write_max_logs bound."""
import random

import pytest

import db_write_ref as ref

T = ref.TOMBSTONE
KEYS = [b"", b"a", b"ab", b"abc", b"b", b"\xff\x00"]


def random_ops(rng, n, keys=KEYS, p_delete=0.4):
    ops = []
    for _ in range(n):
        key = rng.choice(keys)
        if rng.random() < p_delete:
            ops.append((ref.DELETE, key, rng.choice([b"", b"ignored"])))
        else:
            ops.append((ref.PUT, key, rng.choice([b"", b"v", T, b"x" * rng.randrange(40)])))
    return ops


def norm(logs):
    return [[(k, b"" if v is None else bytes(v)) for k, v in lg] for lg in logs]


def sums(ops):
    return (sum(len(k) for _, k, _ in ops), sum(len(v) for _, _, v in ops))


@pytest.mark.parametrize("seed", range(40))
def test_closed_form_equals_the_manager(seed):
    rng = random.Random(seed)
    rotated = extras = 0
    for _ in range(75):
        ops = random_ops(rng, rng.randrange(0, 121))
        mem_max = rng.randrange(40, 1001)
        mem_size0 = rng.choice([0, 0, rng.randrange(0, mem_max + 1), mem_max, mem_max + rng.randrange(1, 50)])
        nodes = [(k, rng.choice([b"n", T])) for k in KEYS if rng.random() < 0.3]
        logs, size = ref.manager_write(ops, mem_size0, mem_max, nodes)
        w = ref.write(ops, mem_size0, mem_max, [k for k, _ in nodes])
        assert norm(w.logs) == norm(logs)
        assert w.size == size
        # nil and the empty value differ in the skiplist, not in the log bytes
        assert [(k, v is None) for lg in w.logs for k, v in lg] == [(k, v is None) for lg in logs for k, v in lg]
        kb, vb = sums(ops)
        assert w.nlog <= ref.max_logs(len(ops), kb, vb, mem_size0, mem_max)
        assert w.log_start[0] == 0 and w.log_start[-1] == len(ops) and len(w.log_start) == w.nlog + 1
        for i, (lg, r) in enumerate(w.main):
            assert w.logs[lg][r] == ref.main_pair(ops[i])
            assert w.log_start[lg] <= i < max(w.log_start[lg + 1], i + 1)
        rotated += w.nlog > 1
        extras += sum(v is None for lg in w.logs for _, v in lg)
    assert rotated > 10 and extras > 10


def test_fit_boundary():
    # est = 16 + 1 + 3 = 20: five fill 100 exactly, the sixth rotates
    ops = [(ref.PUT, b"k", b"abc")] * 6
    assert [len(lg) for lg in ref.write(ops, 0, 100).logs] == [5, 1]
    assert [len(lg) for lg in ref.write(ops, 0, 99).logs] == [4, 2]
    assert [len(lg) for lg in ref.write(ops, 1, 100).logs] == [4, 2]
    for mem_size0, mem_max in ((0, 100), (0, 99), (1, 100)):
        assert norm(ref.manager_write(ops, mem_size0, mem_max)[0]) == norm(ref.write(ops, mem_size0, mem_max).logs)


def test_log0_may_stay_empty_and_an_oversized_op_gets_its_own_log():
    big = (ref.PUT, b"big", b"x" * 200)
    small = (ref.PUT, b"s", b"")
    w = ref.write([big, small, big, small], 0, 50)
    assert [len(lg) for lg in w.logs] == [0, 1, 1, 1, 1] and w.log_start == [0, 0, 1, 2, 3, 4]
    assert norm(ref.manager_write([big, small, big, small], 0, 50)[0]) == norm(w.logs)
    w = ref.write([small], 70, 50)
    assert [len(lg) for lg in w.logs] == [0, 1] and w.size == 17


def test_boundary_delete_puts_the_extra_in_the_old_log():
    ops = [(ref.PUT, b"k", b"v" * 10), (ref.DELETE, b"k", b"")]
    w = ref.write(ops, 0, 30)  # 27, then 30 more: the Delete opens log 1
    assert w.logs == [[(b"k", b"v" * 10), (b"k", None)], [(b"k", T)]]
    assert w.main == [(0, 0), (1, 0)]
    logs, size = ref.manager_write(ops, 0, 30)
    assert norm(logs) == norm(w.logs) and size == w.size == 30
    # the nodes count for log 0 only
    ops = [(ref.DELETE, b"n", b""), (ref.PUT, b"p", b"x" * 40), (ref.DELETE, b"n", b""), (ref.DELETE, b"m", b"")]
    w = ref.write(ops, 0, 60, nodes=[b"n", b"m"])
    assert norm(w.logs) == norm(ref.manager_write(ops, 0, 60, [(b"n", b"1"), (b"m", b"2")])[0])
    # 30 in log 0; 57 rotates; 30 more rotates again; the last 30 fits beside it (60)
    assert [len(lg) for lg in w.logs] == [2, 1, 2] and w.logs[0][0] == (b"n", None)
    assert all(v is not None for lg in w.logs[1:] for _, v in lg)


@pytest.mark.parametrize("seed", range(5))
def test_max_logs_bound(seed):
    rng = random.Random(100 + seed)
    tight = 0
    for _ in range(400):
        n = rng.randrange(0, 60)
        ops = random_ops(rng, n, keys=[b"", b"k", b"key" * 5], p_delete=rng.choice([0, 0.5, 1]))
        mem_max = rng.choice([1, 15, 16, 17, 29, 30, 40, 100, 1000])
        mem_size0 = rng.choice([0, 1, mem_max, mem_max + 1, 5 * mem_max])
        kb, vb = sums(ops)
        bound = ref.max_logs(n, kb, vb, mem_size0, mem_max)
        nlog = ref.write(ops, mem_size0, mem_max).nlog
        assert 1 <= nlog <= bound
        tight += nlog == bound
    assert tight > 0  # n + 1 logs are reached


def test_dict_model():
    ops = [(ref.PUT, b"a", b"1"), (ref.DELETE, b"a", b""), (ref.PUT, b"b", b"2"), (ref.PUT, b"b", b"3")]
    assert ref.dict_model(ops) == {b"a": T, b"b": b"3"}
