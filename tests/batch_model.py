"""Test helper: the batch of texts as ONE text (krep_gpu_search_batch, include/krep_gpu.h "a batch of texts in one scan"), in numpy.

pack(items) joins the items with one '\\n' between neighbours; split(records, items) cuts a record list of the pack back into the
items' own lists; separable(eng, search, A, B) asks the reference itself whether result(A + '\\n' + B) is result(A) followed by
result(B) shifted by |A| + 1 — the property that makes packing exact.  A Search names one input class: the patterns, the reference
build and the file-static only_matching that pick the reference function, and the params.

edge_items(s) and check_batch(gpu, s, items) are what the GPU tests share: the items at the edge lengths, and the comparison of a batch
with the reference and with the operator on each item alone.

TEST INFRASTRUCTURE: imported by the batch tests only (tests/test_batch_*_cpu.py, tests/test_gpu_batch*.py, tests/test_abi_batch.py)."""
from __future__ import annotations

import numpy as np

import oracle_lib as ol
import regex_alt_model
import regex_ext_model
import regex_ref
from krep_amd import abi

NONE = np.zeros((0, 2), dtype=np.uint64)


def as_array(item) -> np.ndarray:
    return item if isinstance(item, np.ndarray) else np.frombuffer(bytes(item), dtype=np.uint8)


def pack(items):
    """-> (the packed text, offsets[n + 1]): item i lies at [offsets[i], offsets[i] + len(i)), offsets[n] = packed size + 1"""
    arrs = [as_array(it) for it in items]
    off = np.zeros(len(arrs) + 1, dtype=np.uint64)
    parts = []
    for i, a in enumerate(arrs):
        if i:
            parts.append(np.full(1, 10, dtype=np.uint8))
        parts.append(a)
        off[i + 1] = off[i] + np.uint64(a.size + 1)
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)), off


def split(records: np.ndarray, items):
    """the records of a pack (item-contiguous, in item order) -> one rebased (n_i, 2) array per item"""
    _, off = pack(items)
    starts = records[:, 0] if records.size else np.zeros(0, dtype=np.uint64)
    out = []
    for i in range(len(items)):
        sel = (starts >= off[i]) & (starts < off[i + 1])
        idx = np.nonzero(sel)[0]
        assert idx.size == 0 or np.array_equal(idx, np.arange(idx[0], idx[0] + idx.size)), "records of an item are not contiguous"
        out.append((records[sel] - off[i]).astype(np.uint64).reshape(-1, 2))
    return out


class Search:
    """One input class: what picks the reference function (patterns, build level, only_matching, regex) and the params."""

    def __init__(self, name, pats, level=abi.REF_AVX2, only_matching=False, regex=False, alphabet=b"ab\n", plants=(),
                 algo_override=abi.ALGO_AUTO, force_no_simd=False, **kw):
        self.name, self.pats, self.level, self.only_matching, self.regex = name, [bytes(p) for p in pats], level, only_matching, regex
        self.alphabet, self.plants, self.kw = alphabet, [bytes(p) for p in plants], kw
        self.algo_override, self.force_no_simd = algo_override, force_no_simd  # (--algo bm / kmp, --no-simd: they pick the function too)

    def with_lines(self) -> "Search":
        s = Search(self.name + " -c", self.pats, self.level, self.only_matching, self.regex, self.alphabet, self.plants,
                   self.algo_override, self.force_no_simd, **self.kw)
        s.kw["count_lines"] = True
        return s

    def params(self) -> abi.Params:
        return abi.Params(self.pats, regex=self.regex, **self.kw)

    def configure(self, eng):
        """the calling thread's configuration of the library: the reference build and the file-static only_matching, algorithm
        override and force_no_simd"""
        eng.set_thread_config(self.config(eng))

    def config(self, eng) -> abi.Config:
        cfg = eng.default_config()
        cfg.reference_simd, cfg.only_matching = self.level, int(self.only_matching)
        cfg.algo_override, cfg.force_no_simd = int(self.algo_override), int(self.force_no_simd)
        return cfg

    def __repr__(self):
        return f"Search({self.name})"


def reference(eng, s: Search, text):
    """what the reference function returns for `text` alone -> (count, positions): the compiled reference where it can be asked
    (oracle_lib.checker, regex_ref), the restatement / the model elsewhere"""
    text = as_array(text)
    if s.regex:
        if regex_ref.available():
            return regex_ref.call(regex_alt_model.joined(s.pats), text, **s.kw)
        return regex_ext_model.run(s.pats, text, **s.kw)
    chk = ol.checker()
    s.configure(eng)
    chk.set_only_matching(s.only_matching)
    chk.lib.ko_set_algo_override(int(s.algo_override))  # (the restatement's copies of the two file-statics: what a function that
    chk.lib.ko_set_force_no_simd(int(s.force_no_simd))  # hands over to another one looks at)
    try:
        p = s.params()
        algo = abi.RA_AHO_CORASICK if len(s.pats) > 1 else eng.mirror_select(p, text.size)
        return chk.call(algo, s.params(), text)
    finally:
        chk.set_only_matching(False)
        chk.lib.ko_set_algo_override(abi.ALGO_AUTO)
        chk.lib.ko_set_force_no_simd(0)
        eng.set_thread_config(None)


def separable(eng, s: Search, A, B) -> bool:
    """result(A + '\\n' + B) == result(A), then result(B) shifted by |A| + 1 (under -c: the counts add up)"""
    A, B = as_array(A), as_array(B)
    ca, pa = reference(eng, s, A)
    cb, pb = reference(eng, s, B)
    cp, pp = reference(eng, s, pack([A, B])[0])
    if cp != ca + cb:
        return False
    if s.kw.get("count_lines"):
        return True
    want = np.concatenate([pa.reshape(-1, 2), pb.reshape(-1, 2) + np.uint64(A.size + 1)]).astype(np.uint64)
    return np.array_equal(pp.reshape(-1, 2), want)


POISON = 0xDEADBEEF


def raw_call(eng, params: abi.Params, items, cfg=None, records=True, want=False):
    """krep_gpu_search_batch itself, with poisoned `results` and a `records` list that already holds one record (start 77, end 78)
    -> (rc, [(count, first_record, n_records)], records->count afterwards, that first record's start afterwards)
    records=False: `records` is NULL (the last two are None).  want=True: two more, the whole record list afterwards as an (n, 2)
    array (None without `records`) and the abi.BatchInfo."""
    import ctypes as C
    arr = (abi.BatchItem * max(len(items), 1))()
    keep = [np.ascontiguousarray(as_array(t)) for t in items]
    for i, k in enumerate(keep):
        arr[i].text, arr[i].len = (k.ctypes.data if k.size else None), k.size
    res = (abi.BatchResult * max(len(items), 1))()
    for r in res:
        r.count = r.first_record = r.n_records = POISON
    rec = None
    if records:
        rec = eng.lib.krep_gpu_match_result_init(16)
        rec.contents.positions[0].start_offset, rec.contents.positions[0].end_offset = 77, 78
        rec.contents.count = 1
    info = abi.BatchInfo()
    dummy = C.c_int(0)
    if params.s.num_patterns > 1 and not params.s.ac_trie:
        params.s.ac_trie = C.cast(C.pointer(dummy), C.c_void_p)  # "caller pre-built the trie", as Engine.search_batch
    try:
        rc = eng.lib.krep_gpu_search_batch(params.ref, C.byref(cfg) if cfg is not None else None, arr, len(items), res, rec, C.byref(info))
        out = (rc, [(r.count, r.first_record, r.n_records) for r in res[:len(items)]], int(rec.contents.count) if rec else None,
               int(rec.contents.positions[0].start_offset) if rec else None)
        return out + ((abi.result_positions(rec) if rec else None), info) if want else out
    finally:
        if rec:
            eng.lib.krep_gpu_match_result_free(rec)
        params.s.ac_trie = None


def random_item(rng: np.random.RandomState, s: Search, n: int) -> np.ndarray:
    """n bytes over the class's alphabet with a few of its plants put in, at the first and the last byte more often than chance"""
    a = np.frombuffer(s.alphabet, dtype=np.uint8)
    t = a[rng.randint(0, len(a), size=n)].astype(np.uint8) if n else np.zeros(0, dtype=np.uint8)
    for _ in range(rng.randint(0, 4) if s.plants else 0):
        p = np.frombuffer(s.plants[rng.randint(len(s.plants))], dtype=np.uint8)
        if p.size > n:
            continue
        where = rng.randint(0, 4)
        at = 0 if where == 0 else n - p.size if where == 1 else rng.randint(0, n - p.size + 1)
        t[at:at + p.size] = p
    return t


EDGE_LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025, 8191, 8192, 8193, 32767, 32768, 32769]


def edge_items(s, seed=11, n_items=48):
    """48 items of the edge lengths, repeated with other contents: a match planted at the first byte, at the last byte and in the
    middle of an item; and, for some neighbours, a match-shaped string SPLIT across them — the end of item k and the start of
    item k + 1 spell the pattern, which must not be found"""
    rng = np.random.RandomState(seed)
    plant = np.frombuffer(s.plants[0], dtype=np.uint8)
    items = []
    for k in range(n_items):
        n = EDGE_LENGTHS[k % len(EDGE_LENGTHS)]
        t = random_item(rng, s, n)
        if n >= plant.size:
            if k % 3 != 2:
                t[:plant.size] = plant
            if k % 4 != 3:
                t[n - plant.size:] = plant
            if n >= 4 * plant.size:
                t[n // 2:n // 2 + plant.size] = plant
        items.append(t)
    if plant.size >= 2:
        h = plant.size // 2
        for k in range(2, n_items - 1, 5):
            a, b = items[k], items[k + 1]
            if a.size >= h and b.size >= plant.size - h:
                a[a.size - h:] = plant[:h]
                b[:plant.size - h] = plant[h:]
    return items


def check_batch(gpu, s, items, single_every=1):
    """the batch's per-item results == the reference on each item alone == the operator on each item alone -> (results, info)"""
    s.configure(gpu)
    try:
        got, info = gpu.search_batch(s.params(), items, want_info=True)
    finally:
        gpu.set_thread_config(None)
    assert len(got) == len(items)
    lines = bool(s.kw.get("count_lines"))
    for i, it in enumerate(items):
        want = reference(gpu, s, it)
        assert got[i][0] == want[0], (s, i, it.size, got[i][0], want[0])
        if lines:
            assert got[i][1].shape == (0, 2)
        else:
            assert np.array_equal(got[i][1], want[1].reshape(-1, 2)), (s, i, it.size)
        if i % single_every == 0:
            s.configure(gpu)
            try:
                one = gpu.search(s.params(), it)
            finally:
                gpu.set_thread_config(None)
            assert gpu.last_status() == abi.STATUS_OK
            assert one[0] == got[i][0] and (lines or np.array_equal(one[1], got[i][1])), (s, i, it.size, one[0], got[i][0])
    assert info.packed_bytes == sum(it.size for it in items) + len(items) - info.scans  # one separator between neighbours of a pack
    return got, info
