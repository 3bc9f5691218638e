"""GPU parity of the LDS-DMA literal kernel in its ONE-PASS records mode (krep_amd/csrc/kg_literal_dma.hip ONEP, kg_scan.hip
lit_dma_one_pass): the scanning waves write the match records at their final index through the ticket -> resolver -> deferred-store
scheme of kg_tickets.h; no info words, no staging slots, no ordering post-pass.  Everything is checked against the compiled reference
(oracle_lib.checker(), the `oracle_engine` fixture) or a closed form.  The mode is taken from ~24 GiB on; small texts reach it through
the test switches krep_gpu_debug_force_rounds(4) (32-KiB units) and $KREP_GPU_LIT_DMA_ALL (tickets of 8 units = 256 KiB then).
How the tests know which road ran: a scan of the new road is ONE launch of lit_scan_dma, and that launch counts as a one-pass launch;
the two-pass road (scan + post_reduce / post_carry / post_offsets / post_gather) launches the kernel without moving that counter.
That is an inference from the host code (lit_dma_one_pass returns before anything of kg_post.hip is reached; the library has no counter
of post-pass launches): what SHOWS that a step holds one kernel and no kg::post_* row is the kernel trace, profiles/r07_literal8_kernel_steady.csv.
Not covered: the spin-limit safety nets of kg_tickets.h (a count or prefix that does not arrive within seconds: a made-up prefix, the scan
flagged and re-run on the two-pass road) — they fire only on a logic error and cannot be provoked without breaking the kernel."""
import os
import time

import numpy as np
import pytest

import cases
from krep_amd import abi

pytestmark = pytest.mark.gpu

UNIT = 32768
TICKET = 8 * UNIT
ALPHA = bytes(range(97, 123)) + b"  \n"


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    return e


@pytest.fixture
def onep(gpu):
    os.environ["KREP_GPU_LIT_DMA_ALL"] = "1"
    os.environ.pop("KREP_GPU_LIT_UPT", None)
    os.environ.pop("KREP_GPU_LIT_DMA_TWO_PASS", None)
    gpu.force_rounds(4)
    yield gpu
    gpu.force_rounds(0)
    gpu.force_literal_dma_grid(0)
    os.environ.pop("KREP_GPU_LIT_DMA_ALL", None)
    os.environ.pop("KREP_GPU_LIT_DMA_TWO_PASS", None)


def _want(gpu, o, text, pat, kw):
    p = abi.Params([pat], **kw)
    return o.call(gpu.mirror_select(p, len(text)), abi.Params([pat], **kw), text)[1].astype(np.int64).reshape(-1, 2)


class Scanner:
    """one plan on device buffers; scan() returns (out, records, one-pass launches, kernel launches, fail-overs) of that scan"""

    def __init__(self, gpu, text, pat, kw, cap):
        import torch
        self.gpu, self.n = gpu, len(text)
        self.buf = torch.from_numpy(np.ascontiguousarray(text)).cuda()
        self.cap = cap
        self.pos = torch.full((2 * cap + 64,), -7, dtype=torch.int64, device="cuda")
        self.plan = gpu.plan(abi.Params([pat], **kw))

    def scan(self, lo=0, hi=None, base=0, cap=None):
        g = self.gpu
        hi = self.n if hi is None else hi
        cap = self.cap if cap is None else cap
        self.pos.fill_(-7)
        b = (g.literal_dma_one_pass_launches(), g.literal_dma_launches(), g.literal_dma_one_pass_failovers())
        out = self.plan.scan(self.buf.data_ptr(), self.n, lo, hi, base, self.pos.data_ptr(), cap, global_len=base + self.n)
        a = (g.literal_dma_one_pass_launches(), g.literal_dma_launches(), g.literal_dma_one_pass_failovers())
        rec = self.pos.cpu().numpy()
        return out, rec, a[0] - b[0], a[1] - b[1], a[2] - b[2]

    def close(self):
        self.plan.close()


def _exact(out, rec, want, cap):
    """count / stored / overflow as on the two-pass road; the first `stored` records exact; nothing written behind them"""
    stored = min(len(want), cap)
    assert out.count == len(want), (out.count, len(want))
    assert out.stored == stored and bool(out.overflow) == (len(want) > cap), (out.stored, stored, out.overflow)
    assert np.array_equal(rec[: 2 * stored].reshape(-1, 2), want[:stored])
    assert (rec[2 * stored:] == -7).all(), "a record was written behind the ones the caller asked for"


def _plant(text, pat, spots):
    m, n = len(pat), len(text)
    p = np.frombuffer(pat, dtype=np.uint8)
    for s in spots:
        if 0 <= s <= n - m:
            text[s:s + m] = p


def _seams(n, m):
    """starts on every seam the kernel has: round end, unit end, ticket end, the ticket's 256-byte tail piece, the ragged end"""
    s = [0, 1, 8192 - m, 8192 - m + 1, 8192 - 1, 8192, 16384 - 3, UNIT - 1, UNIT - m + 2, UNIT, 4 * UNIT - 2, TICKET - 1, TICKET - m,
         TICKET - m + 1, TICKET, TICKET + 1, TICKET + 255 - m, TICKET + 256 - m, TICKET + 256, 2 * TICKET - 7, 2 * TICKET - 1, n - m, n - m - 1,
         n - 8192 - 2, n // 2]
    return [x for x in s if 0 <= x <= n - m]


def _plant_words(text, pat, spots, rot):
    """-w: plants on close seams overwrite each other's neighbours, so every case takes the seams from another one on and skips those
    that touch a plant already made; a plant stands between a blank and a newline, every fourth one behind a letter (rejected)"""
    m, n = len(pat), len(text)
    p = np.frombuffer(pat, dtype=np.uint8)
    taken = []
    for s in spots[rot:] + spots[:rot]:
        if s + m < n and all(abs(s - t) > m + 1 for t in taken):
            text[s:s + m] = p
            text[s + m] = ord("\n")
            if s > 0:
                text[s - 1] = ord("a") if len(taken) % 4 == 3 else ord(" ")
            taken.append(s)


PATS = (b"Qx", b"Zeb", b"WXYZ", b"Kappa", b"Jacket", b"Jacket7", b"Sherlock")


@pytest.mark.parametrize("flavour", ["plain", "ci", "ww"])
def test_every_length_on_every_seam(onep, oracle_engine, flavour):
    gpu = onep
    rng = np.random.RandomState(11)
    kw = dict(plain={}, ci=dict(case_sensitive=False), ww=dict(whole_word=True))[flavour]
    for ni, n in enumerate((2 * TICKET + 4 * 8192 + 5, 3 * TICKET, 3 * TICKET + 8191, 40 * UNIT - 1)):
        for pi, pat in enumerate(PATS):
            if flavour == "ci":
                pat = b"Q" + pat[1:]  # (-i: the prefilter wants a first LETTER that running text rarely holds, in either case)
            m = len(pat)
            text = cases.rand_text(rng, n, ALPHA)
            if flavour == "ww":
                _plant_words(text, pat, _seams(n, m), 3 * pi + ni)
            else:
                _plant(text, pat, _seams(n, m))
            if flavour == "ci":  # some plants in the other case
                for s in _seams(n, m)[::3]:
                    v = text[s:s + m].copy()
                    letter = ((v | 0x20) >= 97) & ((v | 0x20) <= 122)
                    text[s:s + m] = np.where(letter, v ^ 0x20, v)
            want = _want(gpu, oracle_engine, text, pat, kw)
            assert len(want) >= 8, (pat, flavour)
            sc = Scanner(gpu, text, pat, kw, len(want) + 64)
            out, rec, onepass, launches, failed = sc.scan()
            sc.close()
            _exact(out, rec, want, len(want) + 64)
            assert (onepass, launches, failed) == (1, 1, 0), (pat, flavour, n, onepass, launches, failed)


def test_windows_global_base_and_cap(onep, oracle_engine):
    """own_lo / own_hi inside a cell, at round and ticket ends; a GiB boundary inside the text through global_base; pos_cap below the total"""
    gpu = onep
    rng = np.random.RandomState(12)
    n = 20 * UNIT + 4321
    pat = b"Xyz7"
    text = cases.rand_text(rng, n, ALPHA)
    _plant(text, pat, _seams(n, len(pat)) + list(rng.randint(0, n - 4, 200)))
    want = _want(gpu, oracle_engine, text, pat, {})
    sc = Scanner(gpu, text, pat, {}, len(want) + 64)
    base = (3 << 30) - 5 * UNIT - 17  # (the text straddles a GiB boundary of the global offsets, and 2^32 lies behind it)
    for lo, hi in ((0, n), (8191, 8193), (8192, 3 * 8192), (UNIT - 1, TICKET + 1), (100, n - 100), (TICKET - 2, TICKET + 2), (TICKET + 250, n),
                   (5 * UNIT + 1027, 5 * UNIT + 1031), (n - 9000, n)):
        for b in (0, base, (5 << 32) + 3):
            sel = want[(want[:, 0] >= lo) & (want[:, 0] < hi)] + b
            out, rec, onepass, launches, failed = sc.scan(lo, hi, b)
            _exact(out, rec, sel, sc.cap)
            assert (onepass, launches, failed) == (1, 1, 0), (lo, hi, b)
    for cap in (1, 7, 8, 9, 63, 64, 65, len(want) - 1, len(want)):
        out, rec, onepass, launches, failed = sc.scan(0, n, base, cap)
        _exact(out, rec, want + base, cap)
        assert (onepass, launches, failed) == (1, 1, 0), cap
    sc.close()


def test_a_ticket_denser_than_the_list_falls_back(onep, oracle_engine):
    """One ticket holds far more hits than a wave's list (768): counted, not recorded — the scan is handed to the two-pass road (exact
    list, the fail-over counter moves) and the plan does not try the one-pass road again on this text."""
    gpu = onep
    rng = np.random.RandomState(13)
    n = 6 * TICKET + 999
    pat = b"Zq9"
    text = cases.rand_text(rng, n, ALPHA)
    _plant(text, pat, range(2 * TICKET + 100, 2 * TICKET + 100 + 3 * 2000, 3))  # 2000 hits back to back in ticket 2
    _plant(text, pat, _seams(n, 3))
    want = _want(gpu, oracle_engine, text, pat, {})
    assert len(want) >= 2000
    sc = Scanner(gpu, text, pat, {}, len(want) + 64)
    out, rec, onepass, launches, failed = sc.scan()
    _exact(out, rec, want, sc.cap)
    assert (onepass, failed) == (1, 1) and launches >= 2, (onepass, launches, failed)
    for _ in range(2):
        out, rec, onepass, launches, failed = sc.scan()
        _exact(out, rec, want, sc.cap)
        assert (onepass, failed) == (0, 0), "the plan tried the one-pass road again on a text that overflowed it"
    sc.close()


@pytest.mark.timeout(240)
def test_starved_grids(onep):
    """Grids of 1, 2 and 3 workgroups over 4 096 tickets (1 GiB): the exact list (closed form: the generator's plants), no fail-over, in
    seconds — the progress argument of kg_tickets.h with K parked tickets per wave (tests/test_ticket_protocol_parked_model.py)."""
    import torch
    gpu = onep
    n = 1 << 30
    buf = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    gpu.generate(buf.data_ptr(), n, 0, 2, 20261016, b"Sherlock", 10000)  # (kind 2: running text, the pattern planted about once per 10 000 bytes)
    pat = torch.tensor(list(b"Sherlock"), dtype=torch.uint8, device="cuda")
    hit = torch.ones(n - 7, dtype=torch.bool, device="cuda")
    for k in range(8):
        hit &= buf[k:n - 7 + k] == pat[k]
    want = torch.nonzero(hit).flatten()
    del hit
    assert want.numel() > 50_000
    cap = int(want.numel()) + 4096
    pos = torch.empty(2 * cap, dtype=torch.int64, device="cuda")
    b_fail, b_one = gpu.literal_dma_one_pass_failovers(), gpu.literal_dma_one_pass_launches()
    for blocks in (1, 2, 3, 0):
        gpu.force_literal_dma_grid(blocks)
        pos.zero_()
        plan = gpu.plan(abi.Params([b"Sherlock"]))
        t0 = time.time()
        out = plan.scan(buf.data_ptr(), n, 0, n, 0, pos.data_ptr(), cap)
        dt = time.time() - t0
        plan.close()
        assert out.count == out.stored == int(want.numel()) and not out.overflow, blocks
        rec = pos[: 2 * out.stored].view(-1, 2)
        assert torch.equal(rec[:, 0], want) and torch.equal(rec[:, 1], want + 8), blocks
        assert gpu.literal_dma_one_pass_failovers() == b_fail, f"grid of {blocks} workgroups handed over to the two-pass road"
        assert dt < 30, (blocks, dt)
    assert gpu.literal_dma_one_pass_launches() == b_one + 4


def test_three_scans_one_list_and_which_sinks_take_the_road(onep, oracle_engine):
    gpu = onep
    rng = np.random.RandomState(14)
    n = 9 * TICKET + 777
    pat = b"Kappa"
    text = cases.rand_text(rng, n, ALPHA)
    _plant(text, pat, _seams(n, 5) + list(rng.randint(0, n - 5, 900)))
    want = _want(gpu, oracle_engine, text, pat, {})
    sc = Scanner(gpu, text, pat, {}, len(want) + 64)
    lists = []
    for _ in range(3):
        out, rec, onepass, launches, failed = sc.scan()
        _exact(out, rec, want, sc.cap)
        assert (onepass, launches, failed) == (1, 1, 0)
        lists.append(rec.copy())
    assert np.array_equal(lists[0], lists[1]) and np.array_equal(lists[0], lists[2])
    # the switch keeps the two-pass road reachable inside one library: same list, the one-pass counter stands still
    os.environ["KREP_GPU_LIT_DMA_TWO_PASS"] = "1"
    try:
        out, rec, onepass, launches, failed = sc.scan()
        _exact(out, rec, want, sc.cap)
        assert (onepass, launches, failed) == (0, 1, 0)
    finally:
        os.environ.pop("KREP_GPU_LIT_DMA_TWO_PASS", None)
    sc.close()
    # the COUNT sink (no record buffer) and -c keep their roads
    for kw, d_pos in (({}, False), (dict(count_lines=True, only_match=True), False), (dict(count_lines=True), True)):
        sc = Scanner(gpu, text, pat, kw, len(want) + 64)
        before = gpu.literal_dma_one_pass_launches()
        if d_pos:
            out = sc.plan.scan(sc.buf.data_ptr(), n, 0, n, 0, sc.pos.data_ptr(), sc.cap)
        else:
            out = sc.plan.scan(sc.buf.data_ptr(), n, 0, n, 0, 0, 0)
        assert gpu.literal_dma_one_pass_launches() == before, kw
        p = abi.Params([pat], **kw)
        assert out.count == oracle_engine.call(gpu.mirror_select(p, n), abi.Params([pat], **kw), text)[0], kw
        sc.close()
