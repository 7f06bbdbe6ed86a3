"""The lsm_build_sst_views cases (tests/views_cases.py) on the CPU: every
case is well formed, and the case list reaches the paths of
sst_vregion_runs_kernel and sst_vregion_views_kernel (encode.hip) that
tests/test_build_views_gpu.py claims to check.  The coverage assertions are
conditions on the inputs, not measurements: if one fails, a case changed, and
the case is what has to be put right.
"""
import numpy as np
import pytest

import pyoracle as ora
import views_cases as vc

M, K = 20_000, 5  # the shape the whole case list runs at


@pytest.mark.parametrize("name", vc.NAMES)
def test_case_is_well_formed(name):
    c = vc.case(name)
    n = c.n
    assert n <= 1600 and c.nfile <= 6 and c.idx.dtype == np.uint32
    assert c.koff.size == c.voff.size == n + 1 and int(c.file_start[-1]) == n
    assert int(c.idx.max()) < len(c.key_desc) and (c.val_desc is None) == c.kv
    # the views hold the recorded pairs: keys at rec_off + 4, values behind a
    # V descriptor's prefix or behind a KV record's key
    off, ln = c.value_views()
    raw = c.buf.tobytes()
    for i in np.unique(c.idx):
        k, v = c.pairs[i]
        ko = int(c.key_desc["rec_off"][i]) + 4
        assert int(c.key_desc["key_len"][i]) == len(k) and raw[ko:ko + len(k)] == k, i
        assert int(ln[i]) == len(v) and raw[int(off[i]):int(off[i]) + len(v)] == v, i
        if not c.kv:  # caller-made views, and only they, have a prefix that is not the length
            p = int(c.val_desc["rec_off"][i])
            assert (int.from_bytes(raw[p:p + 4], "little") != len(v)) == bool(c.bad[i]), i
    # the packed keys and the offset scans are the selection's
    assert c.keys.tobytes() == b"".join(c.sel_keys) and c.vals.tobytes() == b"".join(c.sel_vals)
    assert np.array_equal(np.diff(c.koff.astype(np.int64)), [len(k) for k in c.sel_keys])
    assert np.array_equal(np.diff(c.voff.astype(np.int64)), [len(v) for v in c.sel_vals])
    long_ok = {"long": {20_000, 70_000}, "long_kv": {20_000}}.get(name, set())
    spans = name == "fix_mix"  # its views over several whole records are as long as those
    assert all(len(v) <= 1024 or len(v) in long_ok or spans for v in c.sel_vals)
    # every expected image decodes back to exactly the selection
    for f, (img, foot) in enumerate(c.expected(M, K)):
        s, e = int(c.file_start[f]), int(c.file_start[f + 1])
        rc, meta, idesc, _, ddesc = ora.sst_decode(img)
        if s == e:
            # an empty data region has size 0, which the reference's decode reads
            # as "to the end of the file" (data.go:51-54) and so runs into the
            # footer: header, filter, footer and index decode, the data does not
            assert rc == 5 and meta.stage == 5 and meta.nidx == 0 and list(foot[[1, 3]]) == [0, 0]
            continue
        assert rc == 0 and meta.stage == 0 and meta.nidx == meta.ndata == e - s, (f, rc, meta.stage)
        b = img.tobytes()
        assert [b[o + 4:o + 4 + l] for o, l in zip(idesc["rec_off"], idesc["key_len"])] == c.sel_keys[s:e], f
        assert [b[o + 4:o + 4 + l] for o, l in zip(ddesc["rec_off"], ddesc["val_len"])] == c.sel_vals[s:e], f


def _all(names):
    return [(n, w) for n in names for w in vc.census(vc.case(n), M, K)]


def test_counts_cover_the_wave_and_chunk_edges():
    for names in (("counts", "counts_chunk"), ("kv_counts", "kv_counts_chunk")):
        sizes = [int(x) for n in names for x in np.diff(vc.case(n).file_start.astype(np.int64))]
        assert sorted(sizes) == [0, 0, 1, 63, 64, 65, 256, 257]
        for n in names:  # the empty file lies between non-empty ones
            d = np.diff(vc.case(n).file_start.astype(np.int64))
            z = int(np.nonzero(d == 0)[0][0])
            assert 0 < z < d.size - 1 and d[z - 1] > 0 and d[z + 1] > 0


def test_v_cases_reach_the_runs_kernel_paths():
    ws = _all(vc.V_NAMES)
    assert any(w["cnt"] == 64 and w["nrun"] == 1 for _, w in ws)
    assert any(w["cnt"] == 64 and w["nrun"] == 64 and w["nfix"] == 0 for n, w in ws if n == "all_breaks")
    per_chunk = vc.CHUNK // vc.WAVE
    assert any(w["continues_prev"] and w["wave"] % per_chunk != 0 for _, w in ws)  # over a wave boundary
    assert any(w["continues_prev"] and w["wave"] % per_chunk == 0 for _, w in ws)  # over a 256-record chunk
    assert {1, 63} <= {w["cnt"] for _, w in ws}
    pairs = {(w["a16"], s) for _, w in ws for s in w["src3"]}
    assert len(pairs) == 64, sorted(set((a, s) for a in range(16) for s in range(4)) - pairs)
    assert any(w["max_bounds"] >= 3 for _, w in ws)
    assert max(w["nslow"] for _, w in ws) <= 130 < vc.SLOW_CAP
    assert any(w["nslow"] >= 128 for n, w in ws if n == "slow_full")
    assert any(w["max_run_rounds"] >= 5 for _, w in ws)
    orders = set().union(*(w["orders"] for n, w in ws if n == "fix_mix"))
    assert {"gb", "bg", "bb"} <= orders


def test_v_cases_reach_what_each_is_named_for():
    cs = {n: vc.census(vc.case(n), M, K) for n in vc.V_NAMES}
    # one_run: single-run 64-record waves at every funnel shift
    one = [w for w in cs["one_run"] if w["cnt"] == 64 and w["nrun"] == 1 and w["file"] > 0]
    assert set().union(*(w["src3"] for w in one)) == {0, 1, 2, 3} and len(one) == 4
    # alternate: runs of 2, 3, 63 and 65 records (65 = 64 up to the wave's end, then 1)
    runs = sorted(len(list(g)) for g in _source_runs(vc.case("alternate"), 1))
    assert {2, 3, 63, 65} <= set(runs)
    # repeat: a record taken twice in succession starts a run each time
    c = vc.case("repeat")
    assert any(a == b for a, b in zip(c.idx, c.idx[1:])) and cs["repeat"][2]["nrun"] == 64
    # empties: runs of 4 bytes with valid prefixes, one run of 4-byte records, fixed 4-byte runs
    assert cs["empties"][0]["max_bounds"] >= 3 and cs["empties"][0]["nfix"] == 0
    assert any(w["nrun"] <= 2 and w["B"] - w["A"] <= 4 * 64 + 200 for w in cs["empties"] if w["file"] == 1)
    assert any(w["nfix"] >= 60 for w in cs["empties"] if w["file"] == 2)
    # sixteen: 16-byte records, each a run, at every A % 16
    assert {w["a16"] for w in cs["sixteen"] if w["nrun"] >= 63} == set(range(16))
    # slow_full: destination starts 13, 14 and 15 modulo 16, two listed segments a record
    assert [(w["a16"], w["nrun"], w["nfix"]) for w in cs["slow_full"]] == [(r, 64, 64) for r in (13, 14, 15)]
    assert all(128 <= w["nslow"] <= 130 for w in cs["slow_full"])
    # align_sweep: the first wave of the 16 files sits at the 16 residues
    heads = {w["a16"] for n in vc.V_NAMES if n.startswith("align_sweep") for w in cs[n] if w["wave"] == 0}
    assert heads == set(range(16))
    # long: the 20,000-byte value first in a 64-record wave, the 70,000-byte one last and alone
    lv = [[len(v) for v in _file_vals(vc.case("long"), f)] for f in range(4)]
    assert lv[0][0] == 20_000 and len(lv[0]) == 64 and lv[1][-1] == 70_000 and len(lv[1]) == 64
    assert lv[2] == [70_000] and 20_000 in lv[3][1:-1] and cs["long"][3]["nrun"] == 1


def _file_vals(c, f):
    return c.sel_vals[int(c.file_start[f]):int(c.file_start[f + 1])]


def _source_runs(c, f):
    """File f's records grouped into stretches that are adjacent in the source
    (not cut at waves)."""
    s, e = int(c.file_start[f]), int(c.file_start[f + 1])
    off, ln = c.value_views()
    run = [s]
    for j in range(s + 1, e):
        a, b = c.idx[j - 1], c.idx[j]
        if int(off[a]) + int(ln[a]) + 4 == int(off[b]):
            run.append(j)
        else:
            yield run
            run = [j]
    yield run


def test_kv_cases_reach_the_views_kernel_paths():
    ws = _all(vc.KV_NAMES)
    pairs = {(w["a4"], s) for _, w in ws for s in w["src4"]}
    assert len(pairs) == 16, pairs
    assert any(w["max_rec_passes"] >= 3 for n, w in ws if n == "long_kv")
    assert {8192, 16384} <= {w["BX"] for n, w in ws if n == "pass_exact"}
    assert any(w["two_rec_dword"] for _, w in ws)
    # long_kv: the long value first in one wave and last in another
    lv = [[len(v) for v in _file_vals(vc.case("long_kv"), f)] for f in range(2)]
    assert lv[0][0] == 20_000 and lv[1][-1] == 20_000 and len(lv[0]) == len(lv[1]) == 64
    # kv_empties: consecutive empty values at every A % 4, so every dword of the
    # stretch holds the ends of two records where A % 4 != 0
    assert {w["a4"] for n, w in ws if n == "kv_empties" and w["wave"] == 0} == {0, 1, 2, 3}
    assert all(w["two_rec_dword"] for n, w in ws if n == "kv_empties" and w["a4"] and w["cnt"] == 64)
    # pass_exact: B cuts the last dword of a full pass, and the first of the next
    assert {8190, 8193} <= {w["BX"] for n, w in ws if n == "pass_exact"}
    # tombs: 13-byte tombstones between values of a multiple of 4 bytes
    t = {len(v) for v in vc.case("tombs").sel_vals}
    assert 13 in t and all(x == 13 or x % 4 == 0 for x in t)


def test_census_depends_on_the_filter_size_only_through_the_data_offset():
    """The other bloom shapes move the data region (the filter block grows),
    which the census must follow: A of a file's first wave is the oracle
    footer's data offset behind the 16-byte aligned image start."""
    c = vc.case("one_run")
    for m, k in ((M, K), (1_600_000, 16), (1_638_401, 7)):
        off, size, data_off = c.layout(m, k)
        assert all(int(o) % 16 == 0 for o in off)
        w0 = [w for w in vc.census(c, m, k) if w["wave"] == 0]
        assert [w["A"] for w in w0] == [int(off[f] + data_off[f]) for f in range(c.nfile)]
