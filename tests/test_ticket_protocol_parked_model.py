"""A MODEL of the ticket -> resolver -> deferred-store protocol as the LDS-DMA literal kernel uses it in its one-pass records mode
(krep_amd/csrc/kg_literal_dma.hip ONEP, kg_tickets.h), scheduled at random on the CPU.  What is new against
tests/test_ticket_protocol_model.py (one parked ticket, its prefix picked up one ticket later):
  * a wave PARKS up to K >= 2 scanned tickets; it publishes every ticket's count when the ticket ends, draws the next ticket where the
    scan of the last one ends, and waits for prefixes only at a FLUSH — when K tickets are parked (or its hit list is full: modelled
    as a random early flush) and when no ticket is left — for all its parked tickets but the one that has just ended (for that one
    too when no ticket is left; the model also runs the variant that never keeps one back);
  * the resolver is the first wave 0 to claim the role and does not scan; any number of workgroups from 1 up is resident, a
    workgroup becomes resident when another has ended, a resident one is never preempted.
Asserted: no schedule leaves a wave waiting for ever, every ticket is scanned once, every prefix is the sum of the counts in front
of it, every ticket is flushed at its prefix.
The negative case is the circular wait this design avoids: counts published only AT the flush, once the wave has seen the counts in
front of each of its parked tickets (in ticket order, across waves).  Wave A holds {0, 3} and wave B {1, 2}: A waits for the counts of
1 and 2, B for the count of 0 — which A publishes only behind its wait.  The model must find that deadlock."""
import random

import pytest

WAVES = 4


class Wave:
    def __init__(self, blk, w):
        self.blk, self.w = blk, w
        self.state = "start"
        self.t = None
        self.left = 0
        self.parked = []
        self.final = False


class Deadlock(AssertionError):
    pass


def held_back_flush_waits(parked, agg):
    """the broken variant's flush: the wave's counts come out only once the counts of all tickets of OTHER waves in front of its
    parked tickets are there; True while it has to wait"""
    return any(agg[u] is None for u in range(max(parked)) if u not in parked)


def run(n_tickets, n_blocks, resident, park_k, seed, publish_at_flush=False, keep_newest=1, scan_steps=3):
    rng = random.Random(seed)
    counter = 0
    claimed = False
    agg = [None] * n_tickets
    pref = [None] * n_tickets
    counts = [rng.randrange(0, 9) for _ in range(n_tickets)]
    scanned = [0] * n_tickets
    flushed = {}
    res_base, res_run = 0, 0
    blocks = [[Wave(b, w) for w in range(WAVES)] for b in range(n_blocks)]
    waiting = list(range(n_blocks))
    res = []

    def done(b):
        return all(x.state == "done" for x in blocks[b])

    def step(x):
        nonlocal counter, claimed, res_base, res_run
        if x.state == "start":
            if x.w == 0 and not claimed:
                claimed = True
                x.state = "resolve"
            else:
                x.state = "draw"
            return True
        if x.state == "resolve":
            moved = False
            while res_base < n_tickets and agg[res_base] is not None:
                pref[res_base] = res_run
                res_run += agg[res_base]
                res_base += 1
                moved = True
            if res_base >= n_tickets:
                x.state = "done"
                return True
            return moved
        if x.state == "draw":
            t = counter
            counter += 1
            if t < n_tickets:
                x.t = t
                x.left = rng.randrange(1, scan_steps + 3)
                x.state = "scan"
            else:
                x.t = None
                x.final = True
                x.state = "flush" if x.parked else "done"
            return True
        if x.state == "scan":
            x.left -= 1
            if x.left > 0:
                return True
            scanned[x.t] += 1
            if not publish_at_flush:
                agg[x.t] = counts[x.t]  # published when the ticket ends, BEFORE the wave waits for anything
            x.parked.append(x.t)
            x.t = None
            full = len(x.parked) >= park_k or rng.random() < 0.15  # (the hit list filled up early)
            x.state = "flush" if full else "draw"
            return True
        if x.state == "flush":
            if publish_at_flush and any(agg[t] is None for t in x.parked):
                # the broken variant: the counts come out only once the flush knows what lies in front of every parked ticket —
                # the counts of all tickets of OTHER waves in front of them, waited for in ticket order
                if held_back_flush_waits(x.parked, agg):
                    return False
                for t in x.parked:
                    agg[t] = counts[t]
                return True
            # the ticket that has just ended stays parked (its prefix may still wait for tickets other waves are finishing), unless
            # nothing is left to scan
            out = x.parked if x.final or keep_newest == 0 else x.parked[:-1]
            if any(pref[t] is None for t in out):
                return False  # waits for the resolver; every count of this wave is out
            for t in out:
                flushed[t] = pref[t]
            x.parked = x.parked[len(out):]
            x.state = ("flush" if x.parked else "done") if x.final else "draw"
            return True
        return False

    for _ in range(400000):
        res = [b for b in res if not done(b)]
        while len(res) < resident and waiting:
            res.append(waiting.pop(0))
        if not res:
            break
        cand = [x for b in res for x in blocks[b] if x.state != "done"]
        rng.shuffle(cand)
        if not any(step(x) for x in cand):
            raise Deadlock(f"no wave can move: tickets={n_tickets} blocks={n_blocks} resident={resident} K={park_k} seed={seed} "
                           f"states={[(x.blk, x.w, x.state, x.t, x.parked) for x in cand]}")
    else:
        raise AssertionError("did not finish")
    assert scanned == [1] * n_tickets
    run_sum = 0
    for t in range(n_tickets):
        assert pref[t] == run_sum, t
        run_sum += counts[t]
        assert flushed.get(t) == pref[t], t


def _configs(count, base):
    for seed in range(count):
        rng = random.Random(base + seed)
        n_tickets = rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 16, 33, 64, 130, 300])
        n_blocks = rng.choice([1, 2, 3, 5, 9, 17])
        resident = min(rng.choice([1, 1, 2, 3, n_blocks]), n_blocks)
        park_k = rng.choice([2, 2, 3, 4, 8, 15, 32])
        yield n_tickets, n_blocks, resident, park_k, seed


def test_no_schedule_leaves_a_wave_waiting():
    n = 0
    for cfg in _configs(800, 20_000):
        run(*cfg, keep_newest=cfg[4] & 1)  # (the kernel keeps the newest parked ticket back; flushing it too is the larger wait)
        n += 1
    assert n == 800


def test_the_circular_wait_constructed():
    """The docstring's case, without the random scheduler: A holds {0, 3}, B holds {1, 2}, both at their flush, no count out.  In the broken
    variant each waits for a count the other holds back — for ever; with every count published at its ticket's end nothing is missing."""
    agg = [None] * 4
    a, b = [0, 3], [1, 2]
    assert held_back_flush_waits(a, agg) and held_back_flush_waits(b, agg)  # neither can move, and nobody else holds a ticket
    agg = [5, 1, 0, 2]  # the shipped order: all four counts are out before either wave waits for anything
    assert not held_back_flush_waits(a, agg) and not held_back_flush_waits(b, agg)


def test_counts_published_only_at_the_flush_deadlock():
    """The negative case: the model itself must be able to see a circular wait.  With counts held back until the flush, and prefixes
    waited for in ticket order across waves, some schedule of some configuration stops for ever."""
    dead = 0
    for cfg in _configs(300, 30_000):
        try:
            run(*cfg, publish_at_flush=True)
        except Deadlock:
            dead += 1
    assert dead > 0
