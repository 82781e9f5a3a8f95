"""Block lengths and fills for the CRC32 tests (tests/test_crc32_host.py on the host, tests/test_bgzf_crc32_gpu.py on the device): every length at which the sliced sum
takes another path, over bytes that show a wrong preset, inversion or shift count."""
import functools
import random

SLICE = 260          # CRC32_SLICE_BYTES of canvas_amd/csrc/crc32_block.hpp: what one lane of the kernel sums


def lengths(sizes=(SLICE,)):
    ns = list(range(0, 71)) + [255, 256, 257, 4095, 4096, 4097, 65535, 65536]
    for s in sizes:
        ns += [s - 1, s, s + 1, 2 * s - 1, 2 * s + 1]
    return sorted(set(ns))


def fills(n, rng):
    """on zeros the sum depends on the length alone"""
    return (("zeros", bytes(n)), ("ones", b"\xff" * n), ("random", rng.randbytes(n)))


@functools.lru_cache(maxsize=None)
def blocks_of_every_length():
    """[(length, kind, bytes)] for every length and fill; made once and left alone"""
    rng = random.Random(20261021)
    return tuple((n, kind, data) for n in lengths() for kind, data in fills(n, rng))
