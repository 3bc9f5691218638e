"""Test helper: the batch of texts as ONE text (krep_gpu_search_batch, include/krep_gpu.h "a batch of texts in one scan"), in numpy.

pack(items) joins the items with one '\\n' between neighbours; split(records, items) cuts a record list of the pack back into the
items' own lists; separable(eng, search, A, B) asks the reference itself whether result(A + '\\n' + B) is result(A) followed by
result(B) shifted by |A| + 1 — the property that makes packing exact.  A Search names one input class: the patterns, the reference
build and the file-static only_matching that pick the reference function, and the params.

TEST INFRASTRUCTURE: imported by tests/test_batch_separable_cpu.py and tests/test_gpu_batch.py only."""
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

    def __init__(self, name, pats, level=abi.REF_AVX2, only_matching=False, regex=False, alphabet=b"ab\n", plants=(), **kw):
        self.name, self.pats, self.level, self.only_matching, self.regex = name, [bytes(p) for p in pats], level, only_matching, regex
        self.alphabet, self.plants, self.kw = alphabet, [bytes(p) for p in plants], kw

    def with_lines(self) -> "Search":
        s = Search(self.name + " -c", self.pats, self.level, self.only_matching, self.regex, self.alphabet, self.plants, **self.kw)
        s.kw["count_lines"] = True
        return s

    def params(self) -> abi.Params:
        return abi.Params(self.pats, regex=self.regex, **self.kw)

    def configure(self, eng):
        """the calling thread's configuration of the library: the reference build and the file-static only_matching"""
        cfg = eng.default_config()
        cfg.reference_simd, cfg.only_matching = self.level, int(self.only_matching)
        eng.set_thread_config(cfg)

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
    try:
        p = s.params()
        algo = abi.RA_AHO_CORASICK if len(s.pats) > 1 else eng.mirror_select(p, text.size)
        return chk.call(algo, s.params(), text)
    finally:
        chk.set_only_matching(False)
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


def raw_call(eng, params: abi.Params, items, cfg=None):
    """krep_gpu_search_batch itself, with poisoned `results` and a `records` list that already holds one record
    -> (rc, [(count, first_record, n_records)], records->count afterwards, that first record's start afterwards)"""
    import ctypes as C
    arr = (abi.BatchItem * max(len(items), 1))()
    keep = [C.create_string_buffer(bytes(t), len(t)) for t in items]
    for i, k in enumerate(keep):
        arr[i].text, arr[i].len = C.addressof(k), len(items[i])
    res = (abi.BatchResult * max(len(items), 1))()
    for r in res:
        r.count = r.first_record = r.n_records = POISON
    rec = eng.lib.krep_gpu_match_result_init(16)
    rec.contents.positions[0].start_offset = 77
    rec.contents.count = 1
    info = abi.BatchInfo()
    try:
        rc = eng.lib.krep_gpu_search_batch(params.ref, C.byref(cfg) if cfg is not None else None, arr, len(items), res, rec, C.byref(info))
        return (rc, [(r.count, r.first_record, r.n_records) for r in res[:len(items)]], int(rec.contents.count),
                int(rec.contents.positions[0].start_offset))
    finally:
        eng.lib.krep_gpu_match_result_free(rec)


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
