"""The grep output of a batch as tests/batch_grep_model.py states it, twice: (a) per item the single-text models on the item alone,
(b) the derivation from the PACK that the device formatters implement (krep_gpu_format_lines_items / _matches_items).  Here, without
a device: (a) == (b) on some hundreds of random batches, and (a) is pinned to the stock CLI run once per file (oracle/_ref/krep;
never -r, whose walk order is not defined) on files whose names have different lengths — plain and --color=always, default, -o and
-c.  Where the CLI cannot be built the digests of its answers in tests/golden/batch_grep_output.json stand in."""
import numpy as np
import pytest

import batch_grep_model as bg
import batch_model as bm
import oracle_lib as ol
import regex_ref
from krep_amd import abi

CLI = ol.ref_cli()
STORE = bg.Store()
S = bm.Search
LETTERS = bytes(range(97, 123)) + b"  \n"


def classes(mode):
    om = mode == "matches"
    out = [
        S("literal", [b"ab"], only_matching=om, force_no_simd=True, alphabet=b"ab \n", plants=[b"ab", b"abab"]),
        S("single byte", [b"a"], only_matching=om, alphabet=b"ab\n", plants=[b"a"]),
        S("-i", [b"abA"], only_matching=om, case_sensitive=False, alphabet=b"abAB \n", plants=[b"aBa"]),
        S("-w", [b"ab"], only_matching=om, whole_word=True, alphabet=b"abc_ \n-", plants=[b"ab", b" ab "]),
        S("nested dictionary", [b"Sherlock", b"lock", b"er"], only_matching=om, alphabet=b"Sherlock \n", plants=[b"Sherlock", b"lock"]),
        S("ab|abc", [b"ab|abc"], only_matching=om, regex=True, alphabet=b"abc\n", plants=[b"abc"]),
    ]
    return [s.with_lines() for s in out] if mode == "count" else out


@pytest.fixture(autouse=True, scope="module")
def _c_locale():
    with regex_ref.c_locale():
        yield


@pytest.fixture(scope="module")
def eng():
    import krep_amd
    e = krep_amd.load()
    yield e
    e.set_thread_config(None)


def random_batch(rng, s):
    n_items = int(rng.randint(1, 9))
    items = []
    for _ in range(n_items):
        n = int(rng.choice([0, 0, 1, 2, 5, 17, 40, 120, 400]))
        t = bm.random_item(rng, s, n)
        if n and rng.randint(3) == 0:
            t[-1] = 10  # a final newline
        if n > 20 and rng.randint(4) == 0:
            t[-int(rng.randint(2, 12)):] = s.alphabet[0]  # a last line without one, where numbers go stale
        items.append(t)
    return items


def answers(eng, s, items):
    """per item what the reference returns: (counts, record lists relative to the item)"""
    got = [bm.reference(eng, s, it) for it in items]
    return [int(c) for c, _ in got], [np.asarray(p, dtype=np.uint64).reshape(-1, 2) for _, p in got]


def names_for(n):
    lens = [1, 15, 16, 17, 3, 40, 2, 255]
    return [(b"f%d" % k + b"x" * 300)[:lens[k % len(lens)]] for k in range(n)]


def test_the_definition_equals_the_pack_derivation(eng):
    rng = np.random.RandomState(20261020)
    done = stale = 0
    for mode in ("lines", "matches"):
        for s in classes(mode):
            for rep in range(30):
                items = random_batch(rng, s)
                _, recs = answers(eng, s, items)
                names = names_for(len(items))
                rec = bg.pack_records(items, recs)
                for color in (False, True) if rep % 3 == 0 else (False,):
                    a, where_a = bg.definition(items, recs, names, mode, color)
                    b, where_b, _ = bg.from_pack(items, rec, names, mode, color)
                    assert a == b, (s, mode, color, [bytes(bm.as_array(i)) for i in items], a[:300], b[:300])
                    assert where_a == where_b, (s, mode, where_a, where_b)
                done += 1
                pack, off = bm.pack(items)
                stale += int(bg.item_tables(pack, off, rec)[5].any())
    assert done >= 300 and stale >= 20, (done, stale)


def test_the_stale_rule_is_per_file():
    """11 records of which 9 lie behind the item's last newline, next to an item with 10: the first prints stale numbers, the second
    true ones, and neither sees the other's newlines"""
    items = [b"xa\nya\n" + b"a" * 9, b"xa\nya\n" + b"a" * 8, b"a" * 12, b"q\n" + b"a" * 11]
    recs = [[(k, k + 1) for k, c in enumerate(t) if c == 97] for t in items]
    names = [b"one", b"two", b"three", b"four"]
    rows = lambda name, nums: b"".join(name + b":%d:a\n" % k for k in nums)  # noqa: E731
    want = rows(b"one", [1, 2] + [2] * 9) + rows(b"two", [1, 2] + [3] * 8) + rows(b"three", [1] * 12) + rows(b"four", [1] * 11)
    a, _ = bg.definition(items, recs, names, "matches")
    b, where, _ = bg.from_pack(items, bg.pack_records(items, recs), names, "matches")
    assert a == want and b == want
    assert [n for _, n in where] == [len(rows(nm, [1] * k)) for nm, k in zip(names, (11, 10, 12, 11))]


def cli_batches():
    """(key, search, mode, items): a few dozen batches, the stale batch among them"""
    rng = np.random.RandomState(77)
    out = []
    for mode in bg.MODES:
        for s in classes(mode):
            for rep in range(2):
                out.append((f"{mode}/{s.name}/{rep}", s, mode, random_batch(rng, s)))
    s = S("single byte", [b"a"], only_matching=True, alphabet=b"ab\n")
    stale = [np.frombuffer(t, dtype=np.uint8) for t in (b"xa\nya\n" + b"a" * 9, b"xa\nya\n" + b"a" * 8, b"", b"x\n" + b"a" * 11, b"b\n")]
    out.append(("matches/stale-per-file", s, "matches", stale))
    return out


def test_the_definition_matches_the_cli_once_per_file(eng, tmp_path):
    batches = cli_batches()
    assert len(batches) >= 36
    for idx, (key, s, mode, items) in enumerate(batches):
        counts, recs = answers(eng, s, items)
        short = names_for(len(items))
        paths = []
        for k, it in enumerate(items):
            (tmp_path / f"b{idx}" / f"i{k}").mkdir(parents=True)
            p = tmp_path / f"b{idx}" / f"i{k}" / short[k].decode()  # (a directory each: two files of a batch may share a name)
            p.write_bytes(bm.as_array(it).tobytes())
            paths.append(p)
        for color in (False, True):
            mine_short, _ = bg.definition(items, recs, short, mode, color, counts)
            live = None
            if CLI:
                full = [str(p).encode() for p in paths]
                mine, _ = bg.definition(items, recs, full, mode, color, counts)
                out = bg.run_cli(CLI, s, mode, color, paths)
                assert out == mine, (key, color, bg.cli_args(s, mode, color), out[:300], mine[:300])
                for f, sh in zip(full, short):  # the stored answer names the files as the batch does, not by where they lay
                    out = out.replace(f, sh)
                live = bg.digest(0, out)
            assert bg.digest(0, mine_short) == STORE.want(key + ("/color" if color else ""), live), key
    STORE.save()
