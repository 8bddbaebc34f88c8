"""INPUTS.md, "Device samples: the rule", restated in Python integers and NumPy: the hypothesis count, the enumerated
pairs, Philox4x32 with 7 rounds, Floyd's algorithm and the sort.  Written from that text, not from
glimpse_amd/csrc/glh_ransac_draw.h: tests/test_ransac_draw_host.py holds the header's CPU program to it number for number,
tests/test_gpu_ransac_draw.py the device.  Nothing here needs a GPU or the library."""
import itertools
import math

import numpy as np

TAG = 0x52414E53  # "RANS"
ROUNDS = 7
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32(counter, key, rounds=ROUNDS):
    """Salmon et al. 2011: four uint64 arrays (or integers) holding 32-bit words -> the four output words, as uint64
    arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in counter)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(rounds):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2  # (32 x 32 bits: no overflow of 64)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(MASK), p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox4x32_integers(counter, key, rounds=ROUNDS):
    """The same in plain Python integers, one block: the check of the array form."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def seed_words(seed):
    assert 0 <= seed < 2 ** 64
    return seed & MASK, seed >> 32


def hypotheses(s, n, iterations):
    """(H_k, enumerated) of a pair of s rows; (0, False) for a pair of n rows or fewer."""
    if s <= n:
        return 0, False
    c = math.comb(s, n)
    return min(iterations, c), c <= iterations


def enumerated(s, n):
    """All combinations in lexicographic order, (C, n) int64."""
    return np.array(list(itertools.combinations(range(s), n)), dtype=np.int64).reshape(-1, n)


def drawn(seed, k, s, n, hyps):
    """The samples of the hypotheses `hyps` (numbers counted from the pair's first) of the drawn pair k of s rows:
    (len(hyps), n) int64, each ascending.  Floyd's algorithm on all hypotheses at once."""
    assert n < s <= 2 ** 31 - 1
    h = np.asarray(hyps, dtype=np.uint64).reshape(-1)
    key = seed_words(seed)
    out = np.zeros((len(h), n), dtype=np.int64)
    words = None
    for i in range(n):
        if i % 4 == 0:
            words = philox4x32((h, np.full(len(h), k, np.uint64), np.full(len(h), i // 4, np.uint64),
                                np.full(len(h), TAG, np.uint64)), key)
        j = s - n + i
        t = ((words[i % 4] * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)  # (a 32-bit word times j + 1 <= 2^31 - 1)
        taken = (out[:, :i] == t[:, None]).any(axis=1)
        out[:, i] = np.where(taken, j, t)
    return np.sort(out, axis=1)


def samples(seed, k, s, n, iterations):
    """What pair k of s rows gets: (H_k, n) int64, or None for a pair of n rows or fewer."""
    count, all_of_them = hypotheses(s, n, iterations)
    if s <= n:
        return None
    if all_of_them:
        return enumerated(s, n)
    return drawn(seed, k, s, n, np.arange(count))
