"""CPU tests of bench_write.py: its command line, its vectorised closed form
against db_write_ref.write, and that its check rejects wrong outputs."""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench_write  # noqa: E402
import db_write_ref as ref  # noqa: E402


def test_cli_parses():
    a = bench_write.parse([])
    assert (a.ops, a.keyspace, a.deletes, a.mem_max, a.steps, a.warmup) == (1_000_000, 4096, 0.10, 2 << 20, 20, 3)
    a = bench_write.parse(["--ops", "1000", "--keyspace", "7", "--deletes", "0.5", "--mem-max", "4096",
                           "--steps", "2", "--warmup", "1", "--repeats", "3", "--out", "x.json"])
    assert (a.ops, a.keyspace, a.deletes, a.mem_max, a.steps, a.warmup, a.repeats, a.out) == \
        (1000, 7, 0.5, 4096, 2, 1, 3, "x.json")
    with pytest.raises(SystemExit):
        bench_write.parse(["--no-such-flag"])


def as_result(want, **change):
    """The closed form dressed as lsm_db_write's read-back."""
    got = SimpleNamespace(overflow=False, nlog=want["nlog"], nrec=want["nrec"], nbytes=want["nbytes"],
                          most_records=want["most"], mem_size=want["mem_size"], log_start=want["log_start"],
                          wal_off=want["wal_off"], wal_len=want["wal_len"], rec_base=want["rec_base"],
                          main_slot=want["main_slot"])
    for k, v in change.items():
        setattr(got, k, v)
    return got


@pytest.mark.parametrize("seed", range(6))
def test_closed_form_equals_the_reference(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    ids, is_del = bench_write.gen_ops(n, int(rng.integers(1, 12)), [0.0, 0.1, 0.5, 1.0, 0.3, 0.2][seed], seed)
    mem_max = int(rng.choice([100, 132, 500, 3000]))
    mem_size0 = int(rng.choice([0, 50, mem_max, mem_max + 1]))
    align = int(rng.choice([1, 16]))
    want = bench_write.closed_form(ids, is_del, mem_size0, mem_max, align)
    ops = [(ref.DELETE if d else ref.PUT, b"k%015d" % i, b"v" * bench_write.VAL_LEN) for i, d in zip(ids, is_del)]
    w = ref.write(ops, mem_size0, mem_max)
    assert want["nlog"] == w.nlog and want["log_start"].tolist() == w.log_start
    assert want["wal_len"].tolist() == [len(b) for b in w.log_bytes()]
    assert want["rec_base"].tolist() == w.rec_base() and want["mem_size"] == w.size
    assert want["main_slot"].tolist() == [w.rec_base()[lg] + r for lg, r in w.main]
    assert int(want["extra"].sum()) == sum(v is None for lg in w.logs for _, v in lg)
    assert all(o % align == 0 for o in want["wal_off"].tolist())
    bench_write.verify(as_result(want), want)


def test_check_rejects_wrong_outputs():
    ids, is_del = bench_write.gen_ops(2000, 50, 0.1)
    want = bench_write.closed_form(ids, is_del, 0, 20000, 16)
    assert want["nlog"] > 5 and want["extra"].any()
    bench_write.verify(as_result(want), want)
    with pytest.raises(AssertionError, match="the log count"):
        bench_write.verify(as_result(want, nlog=want["nlog"] + 1), want)
    with pytest.raises(AssertionError, match="the log count"):
        bench_write.verify(as_result(want, nlog=want["nlog"] - 1), want)
    with pytest.raises(AssertionError, match="the record count"):
        bench_write.verify(as_result(want, nrec=want["nrec"] - 1), want)
    bad = copy.deepcopy(want["wal_len"])
    bad[2] += 1
    with pytest.raises(AssertionError, match="each log's bytes"):
        bench_write.verify(as_result(want, wal_len=bad), want)
    with pytest.raises(AssertionError, match="overflow"):
        bench_write.verify(as_result(want, overflow=True), want)
