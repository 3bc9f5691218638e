"""GPU parity of the LDS-DMA literal kernel's one-pass records mode under the TWO-SIZE ticket map (krep_amd/csrc/kg_tickets.h TkMap,
kg_literal_dma.hip ONEP, kg_scan.hip lit_dma_one_pass): long tickets of 16 or 32 units in front, 8-unit tickets at the end of the text,
a ragged last one.  Record for record and in order against the compiled reference (the `oracle_engine` fixture), as
tests/test_gpu_literal_dma_records.py does for the one-size map; its Scanner and planting helpers are used here.

A large text gets long tickets by its density; texts of 2 MiB get them through krep_gpu_debug_force_literal_dma_tickets(long_units,
n_long) on top of $KREP_GPU_LIT_DMA_ALL and 32-KiB units (krep_gpu_debug_force_rounds(4)).  The shape that has every kind of seam: 60
units = two long tickets of 16, three short ones of 8, a ragged one of 4 whose last unit ends in a partial 8-KiB round (the unit grid comes
in tiles of four units, so a ragged ticket has four).  Which map a launch ran with is read back (krep_gpu_debug_literal_dma_last_tickets)."""
import os

import numpy as np
import pytest

import cases
from test_gpu_literal_dma_records import ALPHA, Scanner, _exact, _plant, _want

pytestmark = pytest.mark.gpu

UNIT = 32768
TICKET = 8 * UNIT
LONG = 16 * UNIT
N = 59 * UNIT + 2 * 8192 + 777  # 60 units: [0,16) [16,32) | [32,40) [40,48) [48,56) | [56,60)
SEAMS = dict(long_long=LONG, long_short=2 * LONG, short_short=2 * LONG + TICKET, short_short2=2 * LONG + 2 * TICKET, short_ragged=2 * LONG + 3 * TICKET)


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    return e


@pytest.fixture
def longtk(gpu):
    os.environ["KREP_GPU_LIT_DMA_ALL"] = "1"
    os.environ.pop("KREP_GPU_LIT_UPT", None)
    os.environ.pop("KREP_GPU_LIT_DMA_TWO_PASS", None)
    gpu.force_rounds(4)
    gpu.force_literal_dma_tickets(16, 2)
    yield gpu
    gpu.force_rounds(0)
    gpu.force_literal_dma_grid(0)
    gpu.force_literal_dma_tickets(0, 0)
    os.environ.pop("KREP_GPU_LIT_DMA_ALL", None)


def _spots(m, k):
    """the pattern across every seam with k of its bytes in front of it; behind a seam; across the end of the 256-byte piece a ticket's
    last round reads behind it; at round and unit ends inside a long ticket; the last start of the text"""
    s = []
    for b in SEAMS.values():
        s += [b - k, b + 16, b + 256 - k, b + 300]
    s += [8192 - k, UNIT - k, 9 * UNIT - k, LONG + 12 * UNIT + 8192 - k, N - m, N - m - 8192 - k, N - 2 * 8192 - 777 - k, 0]
    return [x for x in s if 0 <= x <= N - m]


def _text(rng, pat, k, flavour="plain", extra=()):
    text = cases.rand_text(rng, N, ALPHA)
    spots = _spots(len(pat), k) + list(extra)
    _plant(text, pat, spots)
    if flavour == "ww":  # every plant a word (blank in front, newline behind) but the ones 300 bytes behind a seam: a letter in front
        for s in spots:
            if s + len(pat) < N:
                text[s + len(pat)] = ord("\n")
            if s > 0:
                text[s - 1] = ord("a") if (s - 300) in SEAMS.values() else ord(" ")
    if flavour == "ci":  # some plants in the other case
        for s in spots[::3]:
            v = text[s:s + len(pat)].copy()
            letter = ((v | 0x20) >= 97) & ((v | 0x20) <= 122)
            text[s:s + len(pat)] = np.where(letter, v ^ 0x20, v)
    return text


@pytest.mark.parametrize("flavour", ["plain", "ci", "ww"])
def test_every_seam_by_every_split(longtk, oracle_engine, flavour):
    gpu = longtk
    rng = np.random.RandomState(81)
    kw = dict(plain={}, ci=dict(case_sensitive=False), ww=dict(whole_word=True))[flavour]
    pat = b"Qherlock" if flavour == "ci" else b"Sherlock"
    for k in range(1, 8):
        text = _text(rng, pat, k, flavour)
        want = _want(gpu, oracle_engine, text, pat, kw)
        starts = set(want[:, 0].tolist())
        for name, b in SEAMS.items():  # (the reference agrees that the text holds what the case is about)
            assert b - k in starts and ((b + 300 in starts) == (flavour != "ww")), (name, k)
        sc = Scanner(gpu, text, pat, kw, len(want) + 64)
        out, rec, onepass, launches, failed = sc.scan()
        sc.close()
        _exact(out, rec, want, len(want) + 64)
        assert (onepass, launches, failed) == (1, 1, 0), (flavour, k, onepass, launches, failed)
        assert gpu.literal_dma_last_tickets() == (16, 2)


def test_starved_grids_windows_and_cap(longtk, oracle_engine):
    gpu = longtk
    rng = np.random.RandomState(82)
    pat = b"Sherlock"
    text = _text(rng, pat, 3, extra=list(rng.randint(0, N - 8, 300)))
    want = _want(gpu, oracle_engine, text, pat, {})
    sc = Scanner(gpu, text, pat, {}, len(want) + 64)
    # grids of 1, 2 and 3 workgroups: 3, 7, 11 scanning waves for 6 tickets of two sizes (the progress argument of kg_tickets.h)
    for blocks in (1, 2, 3, 0):
        gpu.force_literal_dma_grid(blocks)
        out, rec, onepass, launches, failed = sc.scan()
        _exact(out, rec, want, sc.cap)
        assert (onepass, launches, failed) == (1, 1, 0), blocks
        assert gpu.literal_dma_last_tickets() == (16, 2)
    # owned windows: the unit grid starts at own_lo, so the map is the window's — (long tickets the window holds, ragged units)
    for lo, hi, n_long in ((1234, 13 * UNIT + 77, 1), (100, 30 * UNIT, 2), (5 * UNIT + 3, 40 * UNIT + 100, 2), (LONG - 5, LONG + 3, 0),
                           (7, N, 2), (3 * UNIT + 1, N - 3 * UNIT, 2)):
        sel = want[(want[:, 0] >= lo) & (want[:, 0] < hi)]
        for base in (0, (5 << 32) + 3):
            out, rec, onepass, launches, failed = sc.scan(lo, hi, base)
            _exact(out, rec, sel + base, sc.cap)
            assert (onepass, launches, failed) == (1, 1, 0), (lo, hi)
            assert gpu.literal_dma_last_tickets() == ((16, n_long) if n_long else (8, 0)), (lo, hi)
    # pos_cap below the total
    for cap in (1, 7, 8, 9, 65, len(want) - 1, len(want)):
        out, rec, onepass, launches, failed = sc.scan(0, N, 0, cap)
        _exact(out, rec, want, cap)
        assert (onepass, launches, failed) == (1, 1, 0), cap
    sc.close()


def test_a_long_ticket_denser_than_the_list_shortens_the_plans_long_ticket(longtk, oracle_engine):
    """One 32-unit ticket holds more than a wave's list (768): the scan is handed to the two-pass road, and the plan's next scans of this
    text run with a 16-unit long ticket, which holds its 400 — the one-pass road stays open."""
    gpu = longtk
    gpu.force_literal_dma_tickets(32, 1)
    rng = np.random.RandomState(83)
    pat = b"Zq9"
    dense = [q * TICKET + 5000 + 1000 * i for q in range(4) for i in range(200)]  # 4 x 200 hits in units 0..31
    text = _text(rng, pat, 2, extra=dense)
    want = _want(gpu, oracle_engine, text, pat, {})
    assert 800 < int(((want[:, 0] < 2 * LONG)).sum()) and int((want[:, 0] < LONG).sum()) < 450
    sc = Scanner(gpu, text, pat, {}, len(want) + 64)
    out, rec, onepass, launches, failed = sc.scan()
    _exact(out, rec, want, sc.cap)
    assert (onepass, failed) == (1, 1) and launches >= 2, (onepass, launches, failed)
    assert gpu.literal_dma_last_tickets() == (32, 1)
    for _ in range(2):
        out, rec, onepass, launches, failed = sc.scan()
        _exact(out, rec, want, sc.cap)
        assert (onepass, launches, failed) == (1, 1, 0), (onepass, launches, failed)
        assert gpu.literal_dma_last_tickets() == (16, 1)
    sc.close()


def test_a_plan_learns_its_density_and_takes_long_tickets(longtk, oracle_engine):
    """No forced map: a plan that knows no density scans with 8-unit tickets; the scan counts 290 hits per MiB, at which a 16-unit ticket
    stays under a quarter of the list and a 32-unit one does not; one workgroup (4 waves) and 164 units leave room for four long tickets
    in front of the 96 units of short ones.  Same records from both maps."""
    gpu = longtk
    gpu.force_literal_dma_tickets(0, 0)
    gpu.force_literal_dma_grid(1)
    rng = np.random.RandomState(84)
    n = 161 * UNIT + 4321
    pat = b"Kappa"
    text = cases.rand_text(rng, n, ALPHA)
    _plant(text, pat, list(rng.randint(0, n - 5, 1480)) + [4 * LONG - 2, 2 * LONG - 3, 4 * LONG + TICKET - 1, n - 5])
    want = _want(gpu, oracle_engine, text, pat, {})
    assert 192 < len(want) / (n / (1 << 20)) <= 384
    sc = Scanner(gpu, text, pat, {}, len(want) + 64)
    maps, lists = [], []
    for _ in range(3):
        out, rec, onepass, launches, failed = sc.scan()
        _exact(out, rec, want, sc.cap)
        assert (onepass, launches, failed) == (1, 1, 0)
        maps.append(gpu.literal_dma_last_tickets())
        lists.append(rec.copy())
    sc.close()
    assert maps == [(8, 0), (16, 4), (16, 4)], maps
    assert np.array_equal(lists[0], lists[1]) and np.array_equal(lists[0], lists[2])
