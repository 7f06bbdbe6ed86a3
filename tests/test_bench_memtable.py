"""bench_memtable.py's host side (no GPU): the log generator really produces
overwrites and deletes, and the closed-form checker rejects wrong outputs."""
import os
import sys

import numpy as np
import pytest

import memtable_ref as ref
import pyoracle as ora

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench_memtable as bm


@pytest.fixture(scope="module")
def log():
    return bm.gen_log(64 * 1024, 5)


def records(buf):
    st, desc, _ = ora.decode_block(ora.GRAMMAR_KV, buf)
    assert st == 0
    raw = buf.tobytes()
    return [(raw[o + 4:o + 4 + kl], raw[o + 8 + kl:o + 8 + kl + vl])
            for o, kl, vl in zip(desc["rec_off"].tolist(), desc["key_len"].tolist(), desc["val_len"].tolist())]


def test_generator_bytes_are_the_records_it_reports(log):
    buf, ids, tomb = log
    recs = records(buf)
    assert buf.size <= 64 * 1024 and len(recs) == ids.size == tomb.size > 1000
    assert [k for k, _ in recs] == [b"k%015d" % i for i in ids.tolist()]
    assert [v == bm.TOMBSTONE for _, v in recs] == tomb.tolist()
    assert all(len(v) == (13 if t else bm.VAL_LEN) for (_, v), t in zip(recs, tomb.tolist()))


def test_generator_overwrites_about_a_third_and_deletes(log):
    _, ids, tomb = log
    n = ids.size
    overwrites = n - np.unique(ids).size
    assert 0.25 * n < overwrites < 0.42 * n
    assert 0.02 * n < int(tomb.sum()) < 0.07 * n
    # some key is overwritten more than once, and some tombstone is itself overwritten
    assert np.bincount(ids).max() >= 3
    uniq, pos, _, _ = bm.expected_window(ids, tomb, bm.ALL)
    assert int(tomb.sum()) > int(tomb[pos].sum()) > 0


@pytest.mark.parametrize("scan", [bm.ALL, bm.RANGESCAN])
def test_checker_accepts_the_reference_and_counts(log, scan):
    buf, ids, tomb = log
    good = ref.order(records(buf), scan)
    assert bm.check_order(ids, tomb, good, scan) == len(good) > 0
    bm.check_counts([len(good), 1, len(good)], [len(good)])
    bm.check_counts([len(good), 1, len(good)], [0, len(good), 0])


def test_checker_rejects_a_swapped_pair(log):
    buf, ids, tomb = log
    bad = ref.order(records(buf), bm.ALL)
    bad[10], bad[11] = bad[11], bad[10]
    with pytest.raises(AssertionError, match="not sorted"):
        bm.check_order(ids, tomb, bad, bm.ALL)


def test_checker_rejects_a_kept_older_duplicate(log):
    buf, ids, tomb = log
    good = ref.order(records(buf), bm.ALL)
    j = next(j for j, p in enumerate(good) if (ids[:p] == ids[p]).any())
    older = int(np.nonzero(ids[:good[j]] == ids[good[j]])[0][-1])
    with pytest.raises(AssertionError, match="last write"):
        bm.check_order(ids, tomb, good[:j] + [older] + good[j + 1:], bm.ALL)
    with pytest.raises(AssertionError, match="delivered twice"):
        bm.check_order(ids, tomb, good[:j] + [older] + good[j:], bm.ALL)


def test_checker_rejects_a_wrong_count(log):
    buf, ids, tomb = log
    good = ref.order(records(buf), bm.ALL)
    with pytest.raises(AssertionError, match="count"):
        bm.check_order(ids, tomb, good[:-1], bm.ALL)
    scan = ref.order(records(buf), bm.RANGESCAN)
    with pytest.raises(AssertionError, match="count"):
        bm.check_order(ids, tomb, good, bm.RANGESCAN)  # the pairs behind the tombstone
    shifted = good[good.index(scan[0]) + 1:][:len(scan)]  # as many pairs, one node further on
    with pytest.raises(AssertionError, match="another key"):
        bm.check_order(ids, tomb, shifted, bm.RANGESCAN)
    for wrong in ([len(good) + 1, 1, len(good)], [len(good), 2, len(good)], [len(good), 1, len(good) - 1]):
        with pytest.raises(AssertionError, match="counts"):
            bm.check_counts(wrong, [len(good)])
