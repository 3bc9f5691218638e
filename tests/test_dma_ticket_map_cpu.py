"""The ticket map of the LDS-DMA literal kernel's one-pass records mode (krep_amd/csrc/kg_tickets.h: tk_map, tk_map_tickets,
tk_map_long_tickets, through krep_gpu_debug_ticket_map / krep_gpu_debug_ticket_map_long_tickets of include/krep_gpu_debug.h).

Tickets of two sizes: the first n_long hold upt_long units, the rest upt = 8, the last one what is left.  The kernel gets a ticket's
units from this function, the host the number of tickets and of long tickets: host logic only, no GPU.  Checked here:
  * for every n_units, upt_long and n_long the tickets partition [0, n_units) exactly, in order, without gaps, and a ticket behind the
    text is empty;
  * the number of long tickets the library chooses leaves a region of short tickets of at least 1.5 x waves x upt_long units at the
    end of the text (rule 2 of the map: the last long ticket ends inside the short ones) and one long ticket per wave in front of it;
  * a text too small for that gets none, which is the one-size map."""
import pytest

UPT = 8


@pytest.fixture(scope="module")
def eng():
    import krep_amd
    return krep_amd.load()


def _check_partition(eng, upt_long, n_long, n_units):
    first, units, n_tk = eng.ticket_map(upt_long, UPT, n_long, n_units, 0)
    assert n_tk == n_long + -(-(n_units - n_long * upt_long) // UPT)
    at = 0
    for t in range(n_tk):
        first, units, k = eng.ticket_map(upt_long, UPT, n_long, n_units, t)
        assert k == n_tk
        assert first == at, (upt_long, n_long, n_units, t)
        want = upt_long if t < n_long else UPT
        assert units == min(want, n_units - at) and units >= 1, (upt_long, n_long, n_units, t)
        assert units == want or t == n_tk - 1, "only the last ticket is ragged"
        at += units
    assert at == n_units
    for t in (n_tk, n_tk + 1, n_tk + 5000):  # a wave that draws behind the text gets nothing
        assert eng.ticket_map(upt_long, UPT, n_long, n_units, t) == (n_units, 0, n_tk)


@pytest.mark.parametrize("upt_long", [8, 16, 32])
def test_tickets_partition_the_units(eng, upt_long):
    for n_units in range(1, 301):
        for n_long in range(0, n_units // upt_long + 1):
            _check_partition(eng, upt_long, n_long, n_units)
        assert eng.ticket_map(upt_long, UPT, n_units // upt_long + 1, n_units, 0) is None  # more long tickets than the text holds
    assert eng.ticket_map(upt_long, 0, 0, 100, 0) is None


def _region(waves, upt_long):
    return -(-3 * waves * upt_long // 2)  # ceil(1.5 x waves x upt_long)


@pytest.mark.parametrize("upt_long", [8, 16, 32])
def test_who_gets_long_tickets(eng, upt_long):
    waves_all = (4, 8, 12, 20, 64, 252, 1024, 2048)
    sizes = set(range(1, 301))
    for waves in waves_all:  # ... and around the sizes at which a text gets its first long tickets, and BASELINE's 32 GiB
        edge = _region(waves, upt_long) + waves * upt_long
        sizes.update(range(max(1, edge - 3), edge + 4))
        sizes.update((edge + upt_long - 1, edge + upt_long, 3 * edge + 5))
    sizes.add(1 << 20)
    for waves in waves_all:
        for n_units in sorted(sizes):
            n_long = eng.ticket_map_long_tickets(n_units, upt_long, UPT, waves)
            if upt_long == UPT:
                assert n_long == 0  # (a long ticket no longer than a short one: the one-size map)
                continue
            room = n_units - _region(waves, upt_long)
            if room < waves * upt_long:
                assert n_long == 0, (n_units, upt_long, waves)  # too small for one long ticket per wave in front of the region
                continue
            assert n_long >= waves
            short = n_units - n_long * upt_long
            assert short >= _region(waves, upt_long), (n_units, upt_long, waves, n_long)
            assert short < _region(waves, upt_long) + upt_long, "one more long ticket would have fitted"
            if n_units <= 300 or n_units == 1 << 20 and waves == 2048:
                first, units, n_tk = eng.ticket_map(upt_long, UPT, n_long, n_units, n_long)
                assert first == n_long * upt_long and n_tk == n_long + -(-short // UPT)
            if n_units <= 300:
                _check_partition(eng, upt_long, n_long, n_units)
    assert eng.ticket_map_long_tickets(1000, 32, UPT, 0) == 0


def test_baseline_shape(eng):
    """32 GiB in 32-KiB units on 512 workgroups: 14.5 long tickets and 6 short ones per wave where the one-size map has 64"""
    n_units, waves = 1 << 20, 2048
    n_long = eng.ticket_map_long_tickets(n_units, 32, UPT, waves)
    assert n_long == (n_units - 98304) // 32 == 29696
    _, _, n_tk = eng.ticket_map(32, UPT, n_long, n_units, 0)
    assert n_tk == 29696 + 98304 // 8
    assert 20 < n_tk / waves < 21
