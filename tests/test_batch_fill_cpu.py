"""The bytes of a pack, every slice (kg::batch_fill through krep_gpu_debug_batch_fill_host, include/krep_gpu_debug.h).

krep_gpu_search_batch never builds the pack on the host: the staging ring asks for bytes [lo, lo + cnt) of it, chunk by chunk and —
for a large chunk — a quarter of the chunk per thread, and kg::batch_fill writes them from the items.  A slice may begin in the middle
of an item, on a separator, or in a run of empty items.  Host logic only, no GPU: the hook builds the offset table as the batch call
does and calls the same function; every slice must equal the same slice of batch_model.pack(items)."""
import numpy as np
import pytest

import batch_model as bm

MIB = 1 << 20
GUARD = 2


@pytest.fixture(scope="module")
def eng():
    import krep_amd
    return krep_amd.load()


def test_every_slice_of_400_small_packs(eng):
    rng = np.random.RandomState(20261019)
    slices = 0
    for k in range(400):
        items = [np.zeros(0, dtype=np.uint8) if rng.randint(3) == 0 else rng.randint(97, 123, size=rng.randint(0, 9)).astype(np.uint8)
                 for _ in range(rng.randint(1, 13))]
        want, off = bm.pack(items)
        assert int(off[-1]) == want.size + 1
        held = eng.batch_items(items)
        for lo in range(want.size + 1):
            for cnt in range(want.size - lo + 1):
                got = eng.batch_fill_host(held, lo, cnt, guard=GUARD)
                assert got is not None, (k, lo, cnt)
                assert np.array_equal(got[GUARD:GUARD + cnt], want[lo:lo + cnt]), (k, [it.tobytes() for it in items], lo, cnt)
                assert np.all(got[:GUARD] == 0xA5) and np.all(got[GUARD + cnt:] == 0xA5), (k, lo, cnt)  # nothing around dst is written
                slices += 1
        # a slice that leaves the pack is refused (2), whatever it would have written
        assert eng.batch_fill_host(held, want.size, 1) is None and eng.batch_fill_host(held, want.size + 1, 0) is None
        assert eng.batch_fill_host(held, 0, want.size + 1) is None
    assert slices > 100_000


def test_slices_of_a_staging_chunk_and_its_four_thread_parts(eng):
    """20 MiB, an empty item, 13 MiB: 33 MiB + 2 packed, so the ring takes one chunk of 32 MiB in four parts of 8 MiB and then the rest"""
    rng = np.random.RandomState(7)
    items = [rng.randint(32, 127, size=20 * MIB).astype(np.uint8), np.zeros(0, dtype=np.uint8), rng.randint(32, 127, size=13 * MIB).astype(np.uint8)]
    want, off = bm.pack(items)
    packed = want.size
    assert packed == 33 * MIB + 2 and want[20 * MIB] == 10 and want[20 * MIB + 1] == 10
    held = eng.batch_items(items)
    chunk = 32 * MIB
    slices = [(q * 8 * MIB, 8 * MIB) for q in range(4)] + [(0, chunk), (chunk, packed - chunk), (0, packed)]
    for sep in (20 * MIB, 20 * MIB + 1):  # a slice that begins ON each separator, and on the byte behind it
        for lo in (sep, sep + 1):
            slices += [(lo, 1), (lo, 2), (lo, 3), (lo, 4096), (lo, packed - lo)]
    slices += [(20 * MIB - 1, 4), (packed - 1, 1), (packed, 0)]
    for lo, cnt in slices:
        got = eng.batch_fill_host(held, lo, cnt, guard=GUARD)
        assert got is not None, (lo, cnt)
        assert np.array_equal(got[GUARD:GUARD + cnt], want[lo:lo + cnt]), (lo, cnt)
        assert np.all(got[:GUARD] == 0xA5) and np.all(got[GUARD + cnt:] == 0xA5), (lo, cnt)
    assert eng.batch_fill_host(held, chunk, packed - chunk + 1) is None
