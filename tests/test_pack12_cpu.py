"""packed12 neighbor-list format (sph-exa_amd/csrc/sx_pack12.hpp) on the host, through sx_pack12_pack / _unpack /
_row_words: entry e of group g sits at bits [12e, 12e + 12) of the group's 96-bit little-endian value (three words),
the last group's tail repeats the last position, a row of ngmax entries takes 3 * ceil(ngmax / 8) words."""
import numpy as np
import pytest

import sphexa_amd as sx


def pack(L, pos):
    pos = np.ascontiguousarray(pos, np.uint32)
    words = np.zeros(3 * ((pos.size + 7) // 8), np.uint32)
    assert L.sx_pack12_pack(pos.ctypes.data, pos.size, words.ctypes.data) == 0
    return words


def unpack(L, words, n):
    out = np.zeros(n, np.uint32)
    assert L.sx_pack12_unpack(words.ctypes.data, n, out.ctypes.data) == 0
    return out


def bits_of(words, k):
    """entry k read from the format's definition: bits [12e, 12e + 12) of group k // 8's little-endian value"""
    g, e = divmod(k, 8)
    v = int(words[3 * g]) | (int(words[3 * g + 1]) << 32) | (int(words[3 * g + 2]) << 64)
    return (v >> (12 * e)) & 0xfff


def lists(rng, cnt):
    """ascending position lists of cnt entries below 4096: random ones, one with 0 and 4095, one with equal
    neighbors at every entry (also across the word boundaries at entries 2 and 5)"""
    if cnt == 0:
        return [np.zeros(0, np.uint32)]
    out = [np.sort(rng.integers(0, 4096, cnt)).astype(np.uint32) for _ in range(3)]
    ext = np.sort(rng.integers(0, 4096, cnt)).astype(np.uint32)
    ext[0], ext[-1] = 0, 4095
    out.append(np.sort(ext))
    out.append(np.repeat(np.sort(rng.integers(0, 4096, (cnt + 1) // 2)), 2)[:cnt].astype(np.uint32))
    out.append(np.full(cnt, 4095, np.uint32))
    out.append(np.zeros(cnt, np.uint32))
    return out


@pytest.mark.parametrize("cnt", list(range(151)) + [256])
def test_round_trip_and_tail(cnt):
    L = sx.lib()
    rng = np.random.default_rng(1000 + cnt)
    for pos in lists(rng, cnt):
        words = pack(L, pos)
        ng = (cnt + 7) // 8
        assert words.size == 3 * ng
        full = unpack(L, words, 8 * ng)
        assert np.array_equal(full[:cnt], pos)
        assert np.all(full[cnt:] == (pos[-1] if cnt else 0))  # the tail repeats the last valid position
        assert [bits_of(words, k) for k in range(8 * ng)] == full.tolist()


def test_row_words():
    L = sx.lib()
    for ngmax in list(range(1, 300)) + [1024]:
        assert L.sx_pack12_row_words(ngmax) == 3 * ((ngmax + 7) // 8)
    assert L.sx_pack12_row_words(150) == 57
