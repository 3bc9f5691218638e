"""Word text with PHRASES planted around ownership cuts, for the multi-pattern scan's patterns of more than 16 bytes.  TEST SUPPORT:
imported by tests/test_long_pattern_cuts_cpu.py (which pins it, no GPU) and tests/test_gpu_long_pattern_cuts.py.

The exact dictionary (krep_amd/csrc/kg_ac_anchor.hip exact_table) enters a pattern of L > 16 bytes by its last 16 bytes, as a stand-in
the level walk has to confirm.  A window [own_lo, own_hi) owns a match by its START, so what matters is where a cut lies between a
phrase's start and its end: a phrase is planted at c - k for every k in -2 .. L + 2 (k = bytes of the phrase in front of the cut c;
1 <= k <= L - 16 is the band in which the end lies 16 .. L - 1 bytes behind the cut, where a stand-in taken for a 16-byte pattern
looks as if it started in the next window).

The expected records come from brute_force(): every occurrence of every pattern by bytes.find, in aho_corasick_search's order
(aho_corasick.c:383-437: END ascending, longest first at one END, a duplicate pattern once per copy)."""
from __future__ import annotations

import functools
import random
from collections import namedtuple

import numpy as np

import wordlist

SEED, LINE = 20260930, 80                 # the word text of tests/test_gpu_wordtext.py
TEXT_LEN = (3 << 20) + 4321
PHRASE_LENS = (17, 20, 24, 40, 70)        # 17: the smallest stand-in (a band of one offset); 70: beyond the level walk's 64-bit depth mask
TWIN_LEN = 27                             # one further phrase: the last 16 bytes of the 24-byte phrase behind another front
WINDOW = 70000                            # bytes of the windows on either side of a cut
UNIT = 16384                              # the scan unit of the multi-pattern kernel (kAcUnitBytes)
SUFFIXES = (b"tion", b"ment", b"ness", b"able", b"ings", b"less")

Plant = namedtuple("Plant", "phrase L k cut start")
Case = namedtuple("Case", "text patterns phrases plants expected")


@functools.lru_cache(maxsize=None)
def _words():
    w = wordlist.word_list()
    return w, wordlist.pack(w)


def in_band(L: int, k: int) -> bool:
    """the cut lies behind the phrase's start and 16 .. L - 1 bytes in front of its (exclusive) end"""
    return 1 <= k <= L - 16


def _fill(rng, by_len, room: int) -> list[bytes]:
    """words and the blank behind each, `room` bytes exactly"""
    out = []
    while room:
        l = rng.choice([x for x in range(4, 11) if x + 1 == room or x + 1 <= room - 5])
        out.append(rng.choice(by_len[l]))
        room -= l + 1
    return out


def make_phrases(words, seed: int = 11):
    """-> (phrases, companions): a phrase of every length in PHRASE_LENS and the twin, words of the list's rare half joined by single
    blanks.  Each phrase ends in a word that ends in a common affix; `companions` holds that last word (a pattern of its own: two
    patterns at one END with different starts) and three more words with the same last four bytes (the reversed trie branches right
    behind the phrase's final gram, which a chain-compressed entry cannot express: the end takes the slow path)."""
    rng = random.Random(seed)
    rare = [w for w in words[len(words) // 2:]]
    by_len = {l: [w for w in rare if len(w) == l] for l in range(4, 11)}
    phrases, companions = [], []
    for i, L in enumerate(PHRASE_LENS):
        suf = SUFFIXES[i]
        ends = [w for w in rare if w.endswith(suf) and 6 <= len(w) <= 9]
        last = rng.choice(ends)
        if L == 24:  # (its last 16 bytes are whole words, so that the twin can put other words in front of them)
            tail = _fill(rng, by_len, 16 - len(last))
            front = _fill(rng, by_len, L - 16)
            twin_front = _fill(rng, by_len, TWIN_LEN - 16)
            assert front != twin_front
            twin = b" ".join(twin_front + tail + [last])
        else:
            tail, front = [], _fill(rng, by_len, L - len(last))
        p = b" ".join(front + tail + [last])
        assert len(p) == L, (L, p)
        phrases.append(p)
        companions += [last] + [w for w in rare if w.endswith(suf) and w != last and len(w) >= 5][:3]
    assert len(twin) == TWIN_LEN and twin[-16:] == phrases[2][-16:] and twin != phrases[2]
    phrases.append(twin)
    return phrases, companions


def dictionaries(words, phrases, companions):
    """-> (base, with_short): 300 rare words + the companions + the phrases, every pattern >= 4 bytes; the same plus a few 1..3-byte
    words (the split road scans the phrases in its long part)."""
    base = wordlist.dictionary(words, "rare", n=300)
    base = base + [c for c in companions if c not in set(base)] + list(phrases)
    assert all(len(p) >= 4 for p in base) and len(set(base)) == len(base)
    short = [w for w in words if len(w) <= 3]
    with_short = base + short[:3] + short[-3:] + [b"of", b"th"]
    return base, with_short


def cuts_for(n_plants: int, text_len: int = TEXT_LEN) -> list[int]:
    """one cut per plant, WINDOW bytes clear of either end of the text: every other one on a multiple of the 16-KiB unit, that
    multiple + 1 or - 1 in turn, the rest at odd offsets"""
    step = (text_len - 2 * WINDOW - 2 * UNIT) // n_plants
    assert step >= UNIT // 2 + 4096 and 2 * step > UNIT + 4096  # snapped neighbours stay apart (see below)
    out = []
    for i in range(n_plants):
        c = WINDOW + UNIT + i * step
        if i % 2 == 0:  # the nearest multiple: moves by <= UNIT / 2, its neighbours at +- step stay >= step - UNIT / 2 away
            c = (c + UNIT // 2) // UNIT * UNIT + (0, 1, -1)[(i // 2) % 3]
        else:
            c |= 1
        out.append(c)
    assert all(b - a > 4096 for a, b in zip(out, out[1:])) and out[0] >= WINDOW and out[-1] + WINDOW <= text_len
    return out


def plant(text: np.ndarray, phrase: bytes, start: int):
    """the phrase at `start`, a blank (or the line's newline) on either side: what is left of the words it cuts stays as shorter words"""
    L = len(phrase)
    text[start:start + L] = np.frombuffer(phrase, dtype=np.uint8)
    for at in (start - 1, start + L):
        if 0 <= at < text.size and text[at] not in (32, 10):
            text[at] = 32


def sweep_plants(phrases, text_len: int = TEXT_LEN) -> list[Plant]:
    """every phrase at cut - k for every k in -2 .. L + 2, each (phrase, k) with a cut of its own"""
    pk = [(pi, k) for pi, p in enumerate(phrases) for k in range(-2, len(p) + 3)]
    random.Random(5).shuffle(pk)  # (every phrase meets every kind of cut)
    cuts = cuts_for(len(pk), text_len)
    return sorted((Plant(pi, len(phrases[pi]), k, c, c - k) for (pi, k), c in zip(pk, cuts)), key=lambda q: q.cut)


def brute_force(text, patterns, case_sensitive: bool = True, whole_word: bool = False) -> np.ndarray:
    """(n, 2) int64 records (start, exclusive end) of every occurrence of every pattern, END ascending, longest first at one END, a
    pattern that is listed twice reported twice.  -i folds ASCII letters on both sides; -w asks for no word character (letter, digit,
    underscore) on either side (is_whole_word_match, krep.h:312-319)."""
    raw = bytes(text)
    if not case_sensitive:
        raw = raw.lower()
    wordc = np.zeros(256, dtype=bool)
    for c in b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_":
        wordc[c] = True
    arr = np.frombuffer(raw, dtype=np.uint8)
    starts, ends = [], []
    for p in patterns:
        p = bytes(p) if case_sensitive else bytes(p).lower()
        at, found = raw.find(p), []
        while at >= 0:
            found.append(at)
            at = raw.find(p, at + 1)
        s = np.asarray(found, dtype=np.int64)
        e = s + len(p)
        if whole_word and s.size:
            left = np.where(s > 0, wordc[arr[np.maximum(s - 1, 0)]], False)
            right = np.where(e < arr.size, wordc[arr[np.minimum(e, arr.size - 1)]], False)
            s, e = s[~left & ~right], e[~left & ~right]
        starts.append(s)
        ends.append(e)
    s, e = np.concatenate(starts), np.concatenate(ends)
    order = np.lexsort((s, e))  # END ascending; at one END the smaller start (the longer pattern) first; stable for copies
    return np.stack([s[order], e[order]], axis=1)


def owned(records: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """the records whose START lies in [lo, hi): what a window of a device scan owns"""
    return records[(records[:, 0] >= lo) & (records[:, 0] < hi)]


def build(engine, with_short: bool = False, frequent: bool = False) -> Case:
    """The sweep text: word text of generator kind 5 with every (phrase, k) planted at a cut of its own, the dictionary, and the
    brute-force records.  `engine`: krep_amd.load() (its host generator needs no GPU).  frequent: 300 FREQUENT words in place of the
    rare ones — a dictionary whose rarest windows are common too keeps its end grams on word text, with the exact dictionary built."""
    words, blob = _words()
    phrases, companions = make_phrases(words)
    base, short = dictionaries(words, phrases, companions)
    if frequent:
        base = [x for x in words[32:2000] if len(x) >= 4][:300] + base[300:]
        assert len(set(base)) == len(base)
    text = engine.generate_host(TEXT_LEN, 0, 5, SEED, blob, LINE).copy()
    plants = sweep_plants(phrases)
    for q in plants:
        plant(text, phrases[q.phrase], q.start)
    pats = short if with_short else base
    return Case(text, pats, phrases, plants, brute_force(text, pats))


def build_duplicate(engine) -> Case:
    """A REAL duplicate — a word of at most 16 bytes that the dictionary lists twice, which the exact dictionary also reports as `multi` —
    planted alone at cut - k for every k in -1 .. L + 1: reported once per copy by the window that owns its start, by no other."""
    words, blob = _words()
    phrases, companions = make_phrases(words)
    base, _ = dictionaries(words, phrases, companions)
    dup = next(p for p in base if 10 <= len(p) <= 16)
    text = engine.generate_host(TEXT_LEN, 0, 5, SEED, blob, LINE).copy()
    ks = list(range(-1, len(dup) + 2))
    plants = [Plant(0, len(dup), k, c, c - k) for k, c in zip(ks, cuts_for(len(ks)))]
    for q in plants:
        plant(text, dup, q.start)
    pats = base + [dup]
    return Case(text, pats, [dup], plants, brute_force(text, pats))


def host_text(base_text: np.ndarray, phrase: bytes, j: int, every: int = 4096):
    """The host-path text: a copy of base_text with the phrase starting at m - j for every multiple m of `every` -> (text, starts)"""
    text = base_text.copy()
    starts = [m - j for m in range(every, text.size - len(phrase) - 1, every)]
    for s in starts:
        plant(text, phrase, s)
    return text, starts
