"""tests/search_ref.py (the reference answer of lsm_search, composed from the
oracle's per-level pieces) against a direct Python restatement of the Go text
over plain dict and list tables: Manager.Search (sstable/manager.go:99-133),
searchFromLevel0 (:160-176), searchFromLevelWithSparseIndex (:178-207) and
searchFromTable (:209-223).  SSTable.MayContain is the oracle's
may_contain_batch per table and the Seek + value the restatement of
tests/test_oracle_level_get.py (both pinned against the Go text there).
CPU only."""
import numpy as np

import pyoracle as ora
import search_ref


def go_get(file, entries, key):
    """Iterator.Seek + Valid + Key == key + Value (index.go:157-181,
    sstable.go:271-296, kv.go:181-200); entries: [(key bytes, offset)]."""
    left, right = 0, len(entries)
    while left < right:
        mid = left + (right - left) // 2
        if entries[mid][0] < key:
            left = mid + 1
        else:
            right = mid
    if left >= len(entries) or entries[left][0] != key:
        return ora.GET_ABSENT, None
    off = entries[left][1]
    if off < 0:
        return ora.GET_SEEK_FAILED, None
    rest = file[off:] if off < len(file) else b""
    if len(rest) < 4:
        return ora.GET_VALUE_LENGTH, None
    n = int.from_bytes(rest[:4], "little")
    if n > 1 << 30:
        return ora.GET_VALUE_TOO_LONG, None
    if len(rest) - 4 < n:
        return ora.GET_VALUE_SHORT, None
    return ora.GET_FOUND, (off, n)


def go_search_from_table(sst, key, i, log):
    """manager.go:209-223 -> (result, view); (GET_ABSENT, None) is (nil, nil)."""
    if not sst["may"][i]:                       # :210 !sst.MayContain(key)
        return ora.GET_ABSENT, None
    r, view = go_get(sst["file"], sst["entries"], key)
    if r == ora.GET_ABSENT:
        log.append(sst["id"])                   # passed MayContain, missed the Seek
    return r, view


def go_search(levels, key, i, log):
    """manager.go:99-133 -> (level, table id, result, view)."""
    for level in range(search_ref.LEVELS):      # :101 minSSTableLevel..maxSSTableLevel
        if level == 0:                          # :109-119
            for sst in levels[0]:               # :164 newest first
                r, view = go_search_from_table(sst, key, i, log)
                if r != ora.GET_ABSENT:         # :166 err != nil, :170 val != nil
                    return 0, sst["id"], r, view
            continue
        sparse = levels[level]                  # :185 (an empty level has no candidate, :194)
        lo, hi = 0, len(sparse)                 # :186 sort.Search(n, MinKey > key)
        while lo < hi:
            h = (lo + hi) >> 1
            if not sparse[h]["min"] > key:
                lo = h + 1
            else:
                hi = h
        index = lo
        if index > 0:                           # :189-191
            index -= 1
        if index < len(sparse):                 # :194
            sst = sparse[index]
            r, view = go_search_from_table(sst, key, i, log)
            if r != ora.GET_ABSENT:             # :197 err != nil, :201 val != nil
                return level, sst["id"], r, view
    return -1, -1, ora.GET_ABSENT, None         # :132


def make_table(keys, vals, m, k, corrupt=None):
    kb, ko = search_ref.csr(keys)
    vb, vo = search_ref.csr(vals)
    img, _ = ora.build_sst(kb if kb.size else np.zeros(1, np.uint8), ko,
                           vb if vb.size else np.zeros(1, np.uint8), vo, 0, len(keys), m=m, k=k)
    img = img.copy()
    if corrupt:
        _, meta, idesc, _, _ = ora.sst_decode(img)
        for j, off in corrupt(img.size, int(meta.idx_off)).items():
            if j < len(idesc):
                at = int(idesc["rec_off"][j]) + 4 + int(idesc["key_len"][j])
                img[at:at + 8] = np.frombuffer(int(off).to_bytes(8, "little", signed=True), np.uint8)
    return img


def test_search_ref_matches_go_restatement():
    rng = np.random.default_rng(21)
    fell_through = ended_by_error = deeper_value_hidden = 0
    for trial in range(30):
        space = [b"k%03d" % i for i in range(120)]
        counts = [int(rng.integers(0, 4))] + [int(rng.integers(0, 4)) if rng.random() < 0.6 else 0
                                              for _ in range(6)]
        if trial == 0:
            counts = [0] * 7
        images = []
        for L, c in enumerate(counts):
            if L == 0:
                sets = [sorted(rng.choice(120, int(rng.integers(0, 40)), replace=False).tolist())
                        for _ in range(c)]
            else:  # disjoint sorted tables: cuts of one sorted draw
                ids = sorted(rng.choice(120, int(rng.integers(c, 60)), replace=False).tolist())
                cuts = sorted(rng.choice(np.arange(1, len(ids)), c - 1, replace=False).tolist()) if c > 1 else []
                sets = [ids[a:b] for a, b in zip([0] + cuts, cuts + [len(ids)])] if c else []
            for t, s in enumerate(sets):
                m, k = (64, 1) if (trial + t) % 2 else (2048, 4)
                corrupt = None
                if trial % 3 == 1 and L <= 1 and t == 0:
                    corrupt = lambda n, idx: {0: -5, 1: n, 2: n - 2, 3: idx}
                images.append(make_table([space[i] for i in s], [b"L%d.%d:%d" % (L, t, i) for i in s],
                                         m, k, corrupt))
        level_start = search_ref.level_starts(counts)
        offs, pos = [], 3
        for im in images:
            offs.append(pos)
            pos += im.size + 5
        buf = np.zeros(pos + 16, np.uint8)
        for o, im in zip(offs, images):
            buf[o:o + im.size] = im
        offs = np.array(offs, np.uint64)
        lens = np.array([im.size for im in images], np.uint64)
        dec = [ora.sst_decode(im) for im in images]
        probes = space + [b"", b"zzz", b"k", b"k000\x00"]
        pb, po = search_ref.csr(probes)
        n = len(probes)
        level, table, res, voff, vlen, _ = search_ref.search(buf, offs, lens, dec, level_start, pb, po, n)
        # the same tree as plain Python tables
        tabs = []
        for t, (im, d) in enumerate(zip(images, dec)):
            file = im.tobytes()
            meta, idesc, ival = d[1], d[2], d[3]
            tabs.append({
                "id": t, "file": file,
                "min": file[int(meta.min_key_off):int(meta.min_key_off) + int(meta.min_key_len)],
                "entries": [(file[int(e["rec_off"]) + 4:int(e["rec_off"]) + 4 + int(e["key_len"])], int(v))
                            for e, v in zip(idesc, ival)],
                "may": ora.may_contain_batch(buf, offs[t:t + 1], [meta], pb, po, 0, n)[:, 0]})
        levels = [tabs[int(level_start[L]):int(level_start[L + 1])] for L in range(search_ref.LEVELS)]
        for i, p in enumerate(probes):
            log = []
            wl, wt, wr, view = go_search(levels, p, i, log)
            assert (level[i], table[i], res[i]) == (wl, wt, wr), (trial, p, level[i], table[i], res[i], wl, wt, wr)
            if view:
                assert voff[i] == offs[wt] + view[0] and vlen[i] == view[1]
            else:
                assert voff[i] == 0 and vlen[i] == 0
            if wr == ora.GET_FOUND and any(t < level_start[wl] for t in log):
                fell_through += 1  # a false positive above, the value from a deeper level
            if wr > ora.GET_FOUND:
                ended_by_error += 1
                later = [t for t in tabs[wt + 1:] if any(e[0] == p for e in t["entries"])]
                deeper_value_hidden += bool(later)
    assert fell_through > 20 and ended_by_error > 5 and deeper_value_hidden > 0


def test_level_starts():
    assert search_ref.level_starts((2, 3, 5, 0, 2, 1, 0)).tolist() == [0, 2, 5, 10, 10, 12, 13, 13]
