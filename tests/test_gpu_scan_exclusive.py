"""The prefix scan of kg_format.hip (scan_exclusive: three hand-written kernels, 2048 words per workgroup, one wave that carries the
workgroup sums 64 at a time) on its own, through krep_gpu_debug_scan_exclusive.  Every formatter, the batch segmentation and the line
analysis call it, but only with what their records happen to hold: more than 64 workgroup sums (n > 131072, the `run` carried between
the rounds of fmt_scan_sums) and a running maximum over input that is not nearly monotone are reached here on purpose.
Expected: numpy's exclusive cumsum (uint64: it wraps mod 2^64 as the kernel's sum does) / maximum.accumulate with 0 in front."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# around the 8 words of a thread, the 512 of a wave, the 2048 of a workgroup, the 64 workgroup sums of one round of the second
# kernel, and a third round of it
SIZES = [0, 1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049, 64 * 2048 - 1, 64 * 2048, 64 * 2048 + 1, 130 * 2048 + 5]
GUARD = 0xA5A5A5A5DEADBEEF


@pytest.fixture(scope="module")
def gpu():
    import krep_amd
    e = krep_amd.load()
    assert e.device_count() >= 1
    return e


def exclusive(a: np.ndarray, take_max: bool) -> np.ndarray:
    out = np.zeros_like(a)
    if a.size > 1:
        out[1:] = (np.maximum.accumulate(a) if take_max else np.cumsum(a, dtype=np.uint64))[:-1]
    return out


def run(gpu, a: np.ndarray, take_max: bool) -> np.ndarray:
    """the hook on `a`; the word behind the output and the input itself must come back untouched"""
    import torch
    n = a.size
    d_in = torch.from_numpy(a.view(np.int64).copy()).cuda() if n else torch.empty(1, dtype=torch.int64, device="cuda")
    d_out = torch.from_numpy(np.full(n + 1, GUARD, dtype=np.uint64).view(np.int64)).cuda()
    gpu.scan_exclusive(d_in.data_ptr(), n, d_out.data_ptr(), take_max)
    got = d_out.cpu().numpy().view(np.uint64)
    assert got[n] == GUARD, (n, take_max, hex(int(got[n])))
    if n:
        assert np.array_equal(d_in.cpu().numpy().view(np.uint64), a)
    return got[:n]


def check(gpu, a: np.ndarray, take_max: bool, what):
    got, want = run(gpu, a, take_max), exclusive(a, take_max)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError((what, a.size, take_max, "first wrong index", int(bad[0]), int(got[bad[0]]), int(want[bad[0]]), bad.size))


def rand_u64(rng, n):
    return (rng.randint(0, 1 << 32, size=n).astype(np.uint64) << np.uint64(32)) | rng.randint(0, 1 << 32, size=n).astype(np.uint64)


@pytest.mark.parametrize("n", SIZES)
def test_sum(gpu, n):
    rng = np.random.RandomState(1000 + n % 997)
    check(gpu, rand_u64(rng, n) >> np.uint64(24), False, "words below 2^40")
    check(gpu, np.ones(n, dtype=np.uint64), False, "all ones")
    a = rand_u64(rng, n)
    a[:2] |= np.uint64(1 << 63)  # (the sum leaves 64 bits at the third word already)
    check(gpu, a, False, "full 64-bit words: the sum wraps")


@pytest.mark.parametrize("n", SIZES)
def test_running_maximum(gpu, n):
    rng = np.random.RandomState(2000 + n % 997)
    a = rand_u64(rng, n) >> np.uint64(3)
    a[rng.rand(n) < 0.5] = 0  # not monotone, and about half of the words the identity
    check(gpu, a, True, "random, half zero")
    check(gpu, np.arange(n, 0, -1, dtype=np.uint64) + np.uint64(1 << 40), True, "descending ramp")
    for at in sorted({0, 2047, 2048, n - 1}):
        if 0 <= at < n:
            one = np.zeros(n, dtype=np.uint64)
            one[at] = (1 << 63) + 12345
            check(gpu, one, True, ("one non-zero word at", at))


def test_refusals(gpu):
    import torch
    import krep_amd
    buf = torch.zeros(16, dtype=torch.int64, device="cuda")
    with pytest.raises(krep_amd.KrepGpuError):  # the scan is not in place
        gpu.scan_exclusive(buf.data_ptr(), 8, buf.data_ptr(), False)
    with pytest.raises(krep_amd.KrepGpuError):
        gpu.scan_exclusive(0, 8, buf.data_ptr(), False)
    gpu.scan_exclusive(0, 0, 0, True)  # nothing to do, nothing touched
