"""CPU tests of bench_get.py's generator and closed-form checker (no GPU): the
probes are the mix they claim to be, the closed form is Manager.Search's
answer (pinned to memtable_search_ref), and the checker rejects a wrong log, a
missed tombstone and a wrong source."""
import numpy as np
import pytest

import bench_get
import bench_memtable
import memtable_search_ref as ref

DESC = np.dtype([("rec_off", "<u8"), ("key_len", "<u4"), ("val_len", "<u4")])


@pytest.fixture(scope="module")
def setup():
    logs = [bench_memtable.gen_log(6000, 40 + w) for w in range(4)]
    offs, pos = [], 0
    for buf, _, _ in logs:
        offs.append(pos)
        pos += (buf.size + 15) // 16 * 16 + 16
    mem_ids = np.unique(np.concatenate([ids for _, ids, _ in logs]))
    tabs = [np.arange(0, 900, 3), np.arange(1, 900, 3), np.arange(300, 1500, 2)]  # two at level 0, one at level 1
    level_start = np.array([0, 2, 3, 3, 3, 3, 3, 3], np.uint32)
    ids, kind = bench_get.gen_probes(3000, mem_ids, np.unique(np.concatenate(tabs)), 7)
    mem = bench_get.expected_memtable([(i, t) for _, i, t in logs], offs, ids)
    tables = bench_get.expected_tables(tabs, [0, 100_000, 200_000], level_start, ids, 1000, 100)
    return logs, offs, mem_ids, tabs, ids, kind, mem, tables


def as_outputs(mem, want):
    val = np.zeros(len(mem[0]), DESC)
    val["rec_off"], val["val_len"] = want[3], want[4]
    return [mem[0].copy(), mem[1].copy(), mem[2].view(np.int32).copy(), want[0].copy(), want[1].copy(),
            want[2].copy(), val.view(np.int32).reshape(-1, 4).copy(), want[5].copy()]


def test_the_probes_are_the_mix_they_claim(setup):
    logs, offs, mem_ids, tabs, ids, kind, mem, tables = setup
    assert [int((kind == k).sum()) for k in (0, 1, 2)] == [1000, 1000, 1000]
    assert np.isin(ids[kind == 0], mem_ids).all()
    assert not np.isin(ids[kind != 0], mem_ids).any()
    assert tables[2][kind == 1].all() and not tables[2][kind == 2].any()
    assert (mem[0][kind == 0] != bench_get.MISS).all() and (mem[0][kind != 0] == bench_get.MISS).all()
    assert {bench_get.VALUE, bench_get.DELETED} <= set(mem[0].tolist())
    assert len(set(mem[1][kind == 0].tolist())) == 4  # every log answers some probe


def test_the_closed_form_is_manager_search(setup):
    logs, offs, _, _, ids, _, mem, _ = setup
    recs = []
    for buf, lid, tomb in logs:
        raw, o, lg = buf.tobytes(), 0, []
        for i, t in zip(lid.tolist(), tomb.tolist()):
            vl = bench_get.TOMB_LEN if t else bench_get.VAL_LEN
            assert raw[o + 4:o + 20] == b"k%015d" % i
            lg.append((raw[o + 4:o + 20], raw[o + 24:o + 24 + vl], o))
            o += 24 + vl
        recs.append(lg)
    plain = [[(k, v) for k, v, _ in lg] for lg in recs]
    tables = [ref.last_positions(lg) for lg in plain]
    for j in range(0, ids.size, 7):
        r, w, pos, value = ref.search(plain, b"k%015d" % int(ids[j]), tables)
        assert (mem[0][j], mem[1][j]) == (r, w)
        if r != ref.MISS:
            assert mem[2][j] == offs[w] // 8 + pos
        if r == ref.VALUE:
            assert mem[3][j] == offs[w] + recs[w][pos][2] + 20 and mem[4][j] == len(value)
        else:
            assert mem[3][j] == 0 and mem[4][j] == 0


@pytest.mark.parametrize("hides", [True, False])
def test_the_checker_accepts_the_answer_and_rejects_the_errors(setup, hides):
    *_, mem, tables = setup
    want = bench_get.expected_get(mem, tables, hides, 100)
    good = as_outputs(mem, want)
    bench_get.check_get(good, mem, want)
    answered = np.flatnonzero(mem[0] == bench_get.VALUE)
    deleted = np.flatnonzero(mem[0] == bench_get.DELETED)
    on_found = np.flatnonzero(want[6] & (want[2] == 1))
    assert answered.size and deleted.size and on_found.size

    bad = as_outputs(mem, want)  # an older log answered
    bad[1][answered[0]] -= 1
    with pytest.raises(AssertionError, match="answering log"):
        bench_get.check_get(bad, mem, want)
    bad = as_outputs(mem, want)  # a tombstone read as a value
    bad[0][deleted[0]] = bench_get.VALUE
    with pytest.raises(AssertionError, match="tombstone"):
        bench_get.check_get(bad, mem, want)
    bad = as_outputs(mem, want)  # a table's value reported as the memtable's
    bad[7][on_found[0]] = bench_get.SRC_MEMTABLE
    with pytest.raises(AssertionError, match="source"):
        bench_get.check_get(bad, mem, want)
    bad = as_outputs(mem, want)  # a key the memtables answered searched in the tables all the same
    bad[4][answered[0]] = 0
    with pytest.raises(AssertionError, match="answering table"):
        bench_get.check_get(bad, mem, want)
    if hides:  # the modes differ exactly on the tombstones some table lies under
        exact = bench_get.expected_get(mem, tables, False, 100)
        differ = np.flatnonzero(exact[5] != want[5])
        assert differ.size and (mem[0][differ] == bench_get.DELETED).all()
