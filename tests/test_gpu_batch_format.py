"""The two formatters over a PACK of items in HBM (krep_gpu_format_lines_items, krep_gpu_format_matches_items; kg_batch_format.hip).
Expected bytes: tests/batch_grep_model.py definition() — per item the single-text model on the item alone with its own name — fed with
the compiled reference's records (batch_model.reference).  The shapes are the smallest at which the kernels can go wrong: item
lengths around the 16-byte chunk, the 1-KiB tile and the 4-KiB newline block, runs of empty items, names that start, end and lie across
chunks and tiles, one item with every record, a line over the 2048 cap, the stale rule at 10 / 11 / 12 records, and the item table on
both sides of its LDS limit.  Each test uses a few MiB at most."""
import ctypes as C

import numpy as np
import pytest

import batch_grep_model as bg
import batch_model as bm
import regex_ref
from krep_amd import abi
from krep_amd.engine import KrepGpuError, line_format, match_format

pytestmark = pytest.mark.gpu

S = bm.Search
TEXT = bytes(range(97, 123)) + b"  \n"
NAME_LENGTHS = [1, 15, 16, 17, 255, 4096]


def classes(om):
    return [
        S("literal", [b"Sherlock"], only_matching=om, alphabet=TEXT, plants=[b"Sherlock"]),
        # (four bytes: under -o a 3-byte pattern goes through memchr_short_search, which the batch rule refuses)
        S("-i", [b"abAb"], only_matching=om, case_sensitive=False, alphabet=b"abAB \n", plants=[b"aBaB"]),
        S("-w", [b"ab"], only_matching=om, whole_word=True, alphabet=b"abc_ \n-", plants=[b"ab", b" ab "]),
        S("nested dictionary", [b"Sherlock", b"lock", b"er"], only_matching=om, alphabet=b"Sherlock \n", plants=[b"Sherlock", b"lock"]),
        S("ab|abc", [b"ab|abc"], only_matching=om, regex=True, alphabet=b"abc\n", plants=[b"abc"]),
    ]


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1 and e.available(), e.unavailable_reason()
    yield e
    e.set_thread_config(None)


def names_for(n):
    """names of the edge lengths, some of them identical for different items"""
    return [(b"n%d/" % (k % 3) + b"x" * 4096)[:NAME_LENGTHS[k % len(NAME_LENGTHS)]] for k in range(n)]  # (k and k + 6: the same name)


def shaped_items(s, seed=5):
    """batch_model.edge_items with runs of empty items in front, in the middle and at the end, some items with a final newline, one of
    newlines only"""
    items = bm.edge_items(s, seed=seed, n_items=28)
    for k in range(3, len(items), 4):
        if items[k].size:
            items[k][-1] = 10
    empty = np.zeros(0, dtype=np.uint8)
    return [empty, empty] + items[:14] + [empty, empty, empty, np.full(5, 10, dtype=np.uint8)] + items[14:] + [empty, empty]


class DevicePack:
    """a pack, its tables, its prefixes and a record list on the device (torch owns the memory), the pack at any alignment"""

    def __init__(self, items, rec, prefixes, misalign=3, poison_pack=False):
        import torch
        pack, off = bm.pack(items)
        self.n_items, self.packed = len(items), int(pack.size)
        buf = np.full(pack.size + 64, 0xA5, dtype=np.uint8)
        if not poison_pack:
            buf[misalign:misalign + pack.size] = pack
        self.t_pack = torch.from_numpy(buf).cuda()
        self.d_pack = self.t_pack.data_ptr() + misalign
        self.t_off = torch.from_numpy(off.astype(np.int64)).cuda()
        blob = b"".join(prefixes)
        poff = np.concatenate([[0], np.cumsum([len(p) for p in prefixes])]).astype(np.int64)
        self.t_blob = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).cuda()
        self.t_poff = torch.from_numpy(poff).cuda()
        self.n = int(rec.shape[0])
        self.t_rec = torch.from_numpy(np.ascontiguousarray(rec, dtype=np.uint64).view(np.int64).reshape(-1).copy()
                                      if self.n else np.zeros(2, dtype=np.int64)).cuda()
        self.view = abi.PackView(self.t_off.data_ptr(), self.n_items, self.t_blob.data_ptr(), self.t_poff.data_ptr())

    def run(self, gpu, mode, fmt, out_misalign=0, capacity=None, item_off=True, guard=32):
        """-> (the out struct, the bytes (None on a size query / overflow), the item offsets, the guard bytes left intact)"""
        import torch
        call = gpu.format_matches_items if mode == "matches" else gpu.format_lines_items
        t_item = torch.full((self.n_items + 1,), -1, dtype=torch.int64, device="cuda") if item_off else None
        d_item = t_item.data_ptr() if item_off else 0
        q = call(self.d_pack, self.packed, self.view, self.t_rec.data_ptr(), self.n, fmt, 0, 0, d_item)
        offs = t_item.cpu().numpy().astype(np.uint64) if item_off else None
        if capacity == 0:
            return q, None, offs, True
        cap = int(q.out_bytes) if capacity is None else capacity
        t_out = torch.full((16 + guard + cap + guard + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        base = t_out.data_ptr()
        at = guard + (out_misalign - (base + guard)) % 16  # (base + at) % 16 == out_misalign, at least `guard` bytes in front
        r = call(self.d_pack, self.packed, self.view, self.t_rec.data_ptr(), self.n, fmt, base + at, cap, d_item)
        host = t_out.cpu().numpy()
        wrote = int(r.out_bytes) if not r.overflow else 0
        intact = bool((host[:at] == 0x5A).all() and (host[at + wrote:] == 0x5A).all())
        return r, (host[at:at + wrote].tobytes() if not r.overflow else None), offs, intact


def formats(mode, color):
    f = match_format(None, color) if mode == "matches" else line_format(None, color)
    f.prefix, f.prefix_len = None, 0
    return f


_REF = {}


def reference_records(gpu, s, items, key):
    """the reference's records per item, computed once per (class, -o) and shared"""
    if key not in _REF:
        _REF[key] = [np.asarray(bm.reference(gpu, s, it)[1], dtype=np.uint64).reshape(-1, 2) for it in items]
    return _REF[key]


def check(gpu, items, recs, names, mode, color, out_misalign=0, capped=None):
    prefixes = [bg.prefix(nm, mode, color) for nm in names]
    want, where = bg.definition(items, recs, names, mode, color)
    dp = DevicePack(items, bg.pack_records(items, recs), prefixes)
    r, got, offs, intact = dp.run(gpu, mode, formats(mode, color), out_misalign)
    assert not r.overflow and int(r.out_bytes) == len(want), (mode, color, int(r.out_bytes), len(want))
    assert got == want, (mode, color, next(k for k in range(len(want)) if got[k:k + 1] != want[k:k + 1]))
    assert intact
    assert offs.tolist() == [o for o, _ in where] + [len(want)]
    if capped is not None:
        assert int(r.capped_lines) == capped
    return r


@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
@pytest.mark.parametrize("mode", ["lines", "matches"])
@pytest.mark.parametrize("idx", range(5), ids=[s.name for s in classes(False)])
def test_edge_shapes(gpu, idx, mode, color):
    s = classes(mode == "matches")[idx]
    items = shaped_items(s)
    recs = reference_records(gpu, s, items, (idx, mode == "matches"))
    assert sum(r.shape[0] for r in recs) > 20
    assert any(r.size and r[0, 0] == 0 for r in recs) and any(r.size and r[-1, 1] == it.size for r, it in zip(recs, items))
    r = check(gpu, items, recs, names_for(len(items)), mode, color, out_misalign=(idx * 5 + 1) % 16)
    if mode == "lines":
        assert int(r.lines) == int(r.lines_total) > 0


def letter_records(items, letter=97):
    return [np.array([(k, k + 1) for k in np.flatnonzero(bm.as_array(t) == letter)], dtype=np.uint64).reshape(-1, 2) for t in items]


@pytest.mark.parametrize("mode", ["lines", "matches"])
def test_skew_one_item_holds_every_record(gpu, mode):
    rng = np.random.RandomState(3)
    free = S("free", [], alphabet=b"xyz\n")
    items = [np.zeros(0, dtype=np.uint8) if k % 2 else bm.random_item(rng, free, int(rng.randint(1, 200))) for k in range(101)]
    items[50] = bm.random_item(rng, S("a", [b"a"], alphabet=b"aab\n"), 20000)
    recs = letter_records(items)
    assert recs[50].shape[0] > 8000 and sum(r.shape[0] for r in recs) == recs[50].shape[0]
    check(gpu, items, recs, names_for(len(items)), mode, False)


@pytest.mark.parametrize("color", [False, True], ids=["plain", "color"])
def test_a_line_over_the_cap(gpu, color):
    """one line with 3000 records, plain (`a`) and overlapping (`aa` under --no-simd: every position), inside one item of a batch"""
    line = b"a" * 3000
    items = [b"xa\n", b"b\n" + line + b"\nxa", b"", b"a"]
    plain = letter_records(items)
    check(gpu, items, plain, names_for(4), "lines", color, capped=1)
    over = [np.array([(k, k + 2) for k in range(len(t) - 1) if t[k:k + 2] == b"aa"], dtype=np.uint64).reshape(-1, 2) for t in items]
    assert over[1].shape[0] == 2999
    check(gpu, items, over, names_for(4), "lines", color, capped=1)


def test_the_stale_rule_per_item(gpu):
    """-o: 10, 11 and 12 records; records behind the last newline with and without an earlier record at or before it; no newline at
    all; the last byte the only newline; a LINE that gains a digit inside an item (9 -> 10, 99 -> 100)"""
    items = [b"xa\nya\n" + b"a" * 8,             # 10 records: true numbers
             b"xa\nya\n" + b"a" * 9,             # 11: the nine behind the last newline print 2
             b"xa\nya\n" + b"a" * 10,            # 12
             b"x\n" + b"a" * 11,                 # all behind the only newline, none in front: the fallback to 1
             b"a" * 12,                          # no newline: true numbers
             b"a" * 12 + b"\n",                  # its last byte is its only newline
             b"a\n" * 12 + b"aa",                # 9 -> 10 inside the item, then stale 12
             b"a\n" * 101 + b"a",                # 99 -> 100, the last one stale
             b"",
             b"a\n" * 9 + b"a"]                  # 10 records with a last line: true numbers
    recs = letter_records(items)
    assert [r.shape[0] for r in recs[:4]] == [10, 11, 12, 11]
    for color in (False, True):
        check(gpu, items, recs, names_for(len(items)), "matches", color)
    got, _ = bg.definition(items, recs, [b"f"] * len(items), "matches")
    assert b"f:2:a\n" * 9 in got and b"f:100:a\n" in got


@pytest.mark.parametrize("n_items", [4095, 4096, 4097])
@pytest.mark.parametrize("mode", ["lines", "matches"])
def test_item_table_on_both_sides_of_the_lds_limit(gpu, n_items, mode):
    rng = np.random.RandomState(n_items)
    texts = [b"", b"a", b"ba\n", b"xa\na", b"zz", b"a\n\na"]
    items = [texts[int(k)] for k in rng.randint(0, len(texts), size=n_items)]
    items[-1] = b"qa"
    recs = letter_records(items)
    names = [b"%d" % (k % 97) for k in range(n_items)]
    lds0, glob0 = gpu.batch_format_launches()
    check(gpu, items, recs, names, mode, False)
    lds1, glob1 = gpu.batch_format_launches()
    # which road ran: the table has n_items + 1 entries, 4096 of them fit (two calls: the size query and the write)
    assert (lds1 - lds0, glob1 - glob0) == ((2, 0) if n_items + 1 <= 4096 else (0, 2))


ITEMS = [b"xa\nya", b"", b"aa\n", b"ba"]


def refused(gpu, mode, rec, items=ITEMS, off=None, poff=None, fmt=None, n=None):
    """a hand-made list (or table) must be refused: the pack holds poison, the output stays untouched"""
    import torch
    dp = DevicePack(items, np.array(rec, dtype=np.uint64).reshape(-1, 2), [b"f:"] * len(items), poison_pack=True)
    if off is not None:
        dp.t_off = torch.from_numpy(np.array(off, dtype=np.int64)).cuda()
    if poff is not None:
        dp.t_poff = torch.from_numpy(np.array(poff, dtype=np.int64)).cuda()
    dp.view = abi.PackView(dp.t_off.data_ptr(), dp.n_items, dp.t_blob.data_ptr(), dp.t_poff.data_ptr())
    if n is not None:
        dp.n = n
    t_out = torch.full((256,), 0x5A, dtype=torch.uint8, device="cuda")
    call = gpu.format_matches_items if mode == "matches" else gpu.format_lines_items
    with pytest.raises(KrepGpuError):
        call(dp.d_pack, dp.packed, dp.view, dp.t_rec.data_ptr(), dp.n, fmt, t_out.data_ptr(), 256, 0)
    assert bool((t_out.cpu().numpy() == 0x5A).all())
    return gpu.last_error()


@pytest.mark.parametrize("mode", ["lines", "matches"])
def test_hand_made_lists_are_refused_before_the_pack_is_read(gpu, mode):
    # the pack is "xa\nya" '\n' "" '\n' "aa\n" '\n' "ba": items at 0, 6, 7, 11; separators at 5, 6, 10; 13 bytes
    assert bm.pack(ITEMS)[1].tolist() == [0, 6, 7, 11, 14]
    assert "ascending" in refused(gpu, mode, [(4, 5), (1, 2)])                # not ascending in start
    assert refused(gpu, mode, [(1, 0)])                                          # end < start
    assert "inside one item" in refused(gpu, mode, [(5, 6)])                    # on the separator behind item 0
    assert refused(gpu, mode, [(6, 7)])                                          # on the separator that is the empty item's
    assert refused(gpu, mode, [(10, 11)])                                        # on the separator behind item 2
    assert refused(gpu, mode, [(13, 14)]) and refused(gpu, mode, [(1 << 40, (1 << 40) + 1)])  # >= packed_len
    assert refused(gpu, mode, [(4, 6)]) and refused(gpu, mode, [(8, 12)])      # the end lies behind the item's end
    assert "offset table" in refused(gpu, mode, [(1, 2)], off=[0, 7, 6, 11, 14])  # not ascending
    assert refused(gpu, mode, [(1, 2)], off=[0, 6, 7, 11, 15])                  # the last entry is not packed_len + 1
    assert refused(gpu, mode, [(1, 2)], off=[1, 6, 7, 11, 14])                  # does not begin at 0
    assert refused(gpu, mode, [(1, 2)], poff=[0, 2, 1, 4, 6])                   # the prefix table is not ascending
    assert refused(gpu, mode, [(1, 2)], poff=[0, 2, 4, 6, 8 + (1 << 20)])       # a prefix of more than 2^20 bytes
    assert "records" in refused(gpu, mode, [(1, 2)], n=1 << 40)                 # n >= 2^40
    long_fmt = (abi.MatchFormat(b"", b"x" * ((1 << 20) + 1)) if mode == "matches" else abi.LineFormat(b"", b"x" * ((1 << 20) + 1)))
    assert "format string" in refused(gpu, mode, [(1, 2)], fmt=long_fmt)
    with_prefix = abi.MatchFormat(b"f:") if mode == "matches" else abi.LineFormat(b"f:")
    assert "prefix" in refused(gpu, mode, [(1, 2)], fmt=with_prefix)


@pytest.mark.parametrize("mode", ["lines", "matches"])
def test_size_query_overflow_alignment_and_no_item_offsets(gpu, mode):
    items = [b"xa\nya", b"", b"aa\n", b"ba", b"zz"]
    recs = letter_records(items)
    names = [b"one", b"two", b"three", b"four", b"five"]
    want, where = bg.definition(items, recs, names, mode, True)
    dp = DevicePack(items, bg.pack_records(items, recs), [bg.prefix(nm, mode, True) for nm in names], misalign=7)
    fmt = formats(mode, True)
    q, none, offs, _ = dp.run(gpu, mode, fmt, capacity=0)  # the size query: the item offsets are valid then too
    assert none is None and int(q.out_bytes) == len(want) and not q.overflow
    assert offs.tolist() == [o for o, _ in where] + [len(want)]
    r, none, offs, intact = dp.run(gpu, mode, fmt, capacity=len(want) - 1)  # too small: overflow with valid sizes, nothing written
    assert r.overflow and none is None and int(r.out_bytes) == len(want) and intact
    assert offs.tolist() == [o for o, _ in where] + [len(want)]
    for mis in range(1, 16):  # d_out at every odd offset inside a 16-byte chunk, guard bytes on both sides
        r, got, _, intact = dp.run(gpu, mode, fmt, out_misalign=mis, item_off=False)  # (and d_item_out_off == NULL)
        assert got == want and intact, mis
    # n == 0: the sizes stay 0 and every item offset is 0
    empty = DevicePack(items, bm.NONE, [b"f:"] * len(items))
    r, got, offs, intact = empty.run(gpu, mode, fmt, capacity=64)
    assert int(r.out_bytes) == 0 and got == b"" and intact and offs.tolist() == [0] * (len(items) + 1)
