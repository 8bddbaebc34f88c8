"""The samples of `ransac_pairs(samples="device")` on the CPU (INPUTS.md, "Device samples: the rule").

tests/hostcheck/ransac_draw_hostcheck.cpp, a stand-alone program, drives the headers the library includes
(glimpse_amd/csrc/glh_ransac_draw.h and the plan checks of glh_ransac_plan.h that serve glh_calib_ransac_groups_drawn).  It
is built with AddressSanitizer and UndefinedBehaviorSanitizer and run directly; nothing is loaded into Python.  What it
prints is compared here, number for number, with tests/ransac_draw_restated.py (the draws), `math.comb` (the counts) and
`itertools.combinations` (the enumerations).

The statistics of the rule are checked on the restatement: the device is held to it bit for bit
(tests/test_gpu_ransac_draw.py), so they need no GPU.  The seeds are fixed; SEEDS_REPLACED lists those that had to be
replaced because the restatement failed a bound with them (none so far)."""
import functools
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from tests import ransac_draw_restated as rd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostcheck", "ransac_draw_hostcheck.cpp")
OUT = os.path.join(ROOT, "tests", "hostcheck", "_build", "ransac_draw_hostcheck")
SEED = 0x00C0FFEE << 32 | 0x9E3779B9  # (ransac_draw_hostcheck.cpp: SEED1, SEED0)
LIMIT = 2 ** 31 - 1
SIZES = (13, 63, 64, 65, 257, 2 ** 20, LIMIT)  # and n + 1
NS = (1, 2, 4, 5, 12, 40, 65)
UNIFORMITY_SEED = 20261020
SEEDS_REPLACED = {}
CHI2_999 = {14: 36.12, 99: 148.23}  # the 99.9 % quantiles of chi-square by degrees of freedom


@functools.lru_cache(maxsize=None)
def program_lines():
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    csrc = os.path.join(ROOT, "glimpse_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, name) for name in ("glh_ransac_draw.h", "glh_ransac_plan.h", "glh_calib.h", "glh_math.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", OUT, SRC], check=True)
    run = subprocess.run([OUT], capture_output=True, text=True)
    lines = run.stdout.strip().split("\n")
    print("\n".join(line for line in lines if line.split(" ")[0] not in ("draw", "count", "enum")), run.stderr)
    assert run.returncode == 0 and lines[-1] == "ok" and not run.stderr.strip()
    return lines


def records(word):
    """[(the integers before the colon, those after it)] of the program's lines that begin with `word`."""
    out = []
    for line in program_lines():
        if line.startswith(word + " "):
            head, tail = line[len(word):].split(":")
            out.append(([int(v) for v in head.split()], [int(v) for v in tail.split()]))
    return out


def test_the_program_runs_clean_under_the_sanitizers_and_every_refusal_holds():
    """Its own checks: every sample n distinct ascending rows below s and nothing written beside it, every refusal of the
    plan that the drawn call added, the calls beside each that are served."""
    assert program_lines()[-1] == "ok"


def test_the_draws_equal_the_restatement_number_for_number():
    got = records("draw")
    shapes = sorted({(s, n) for (s, n, _, _), _ in got})
    assert shapes == sorted({(s, n) for n in NS for s in SIZES + (n + 1,) if s > n})
    assert len(got) == len(shapes) * 3 * 7
    different = []
    for (s, n), group in itertools.groupby(sorted(got), key=lambda r: tuple(r[0][:2])):
        group = list(group)
        for k in sorted({head[2] for head, _ in group}):
            mine = [(head[3], rows) for head, rows in group if head[2] == k]
            want = rd.drawn(SEED, k, s, n, [h for h, _ in mine])
            for (h, rows), w in zip(mine, want):
                assert len(rows) == n and len(set(rows)) == n and rows == sorted(rows) and 0 <= rows[0] and rows[-1] < s
                if rows != [int(v) for v in w]:
                    different.append((s, n, k, h))
    assert not different, different


def capped_comb(s, n, cap):
    """min(C(s, n), cap + 1) from math.comb.  A coefficient with min(n, s - n) > 64 is not computed: C(s, m) grows with m up
    to s / 2, so it is at least C(s, 64), and that must exceed the cap for this shortcut to be taken."""
    if n > s:
        return 0
    m = min(n, s - n)
    if m > 64:
        assert math.comb(s, 64) > cap
        return cap + 1
    return min(math.comb(s, m), cap + 1)


def test_the_count_is_the_exact_binomial_coefficient_capped_at_iterations():
    got = records("count")
    assert len(got) > 8 * sum(s + 1 for s in range(1, 41))  # (the program's grid: s to 40, n to s + 1, eight caps; and more)
    seen = set()
    for (s, n, iterations), (hyps, enumerated, c) in got:
        want = capped_comb(s, n, iterations)
        assert c == want, (s, n, iterations)
        if s <= n:
            assert (hyps, enumerated) == (0, 0), (s, n, iterations)
            continue
        assert hyps == min(iterations, want) and enumerated == (want <= iterations), (s, n, iterations)
        if min(n, s - n) <= 64:
            assert (hyps, bool(enumerated)) == rd.hypotheses(s, n, iterations), (s, n, iterations)
        exact = math.comb(s, n) if min(n, s - n) <= 64 else None
        seen.add("C == iterations" if exact == iterations else "C == iterations + 1" if exact == iterations + 1 else "")
        seen.add("n > s / 2" if 2 * n > s and exact is not None and exact > 1 else "")
        seen.add("no overflow" if (s, n) == (LIMIT, 64) else "")
    assert {"C == iterations", "C == iterations + 1", "n > s / 2", "no overflow"} <= seen


def test_the_enumeration_is_itertools_combinations():
    got = records("enum")
    assert len(got) >= 10
    for (s, n, count), rows in got:
        # (itertools holds its pool in memory: of the largest pair only the first combinations are asked for, in which the
        # last place alone moves, and those are the first of any pool of count + n rows or more)
        pool = s if s <= 10 ** 6 else count + n
        want = list(itertools.islice(itertools.combinations(range(pool), n), count))
        assert len(want) == count and rows == [v for c in want for v in c], (s, n, count)
    full = [(s, n) for (s, n, count), _ in got if count == math.comb(s, n) and count > 1]
    assert len(full) >= 5
    assert np.array_equal(rd.samples(0, 0, 6, 3, 20), np.array(list(itertools.combinations(range(6), 3))))


def test_philox_known_answers_and_the_two_forms_of_the_restatement():
    """Random123's known-answer vectors for philox4x32_10 (kat_vectors), and the array form against the integer form at 7
    rounds on assorted counters."""
    ones = 0xFFFFFFFF
    pi = ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))
    known = [(((0, 0, 0, 0), (0, 0)), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
             (((ones,) * 4, (ones, ones)), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
             ((pi[0], pi[1]), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for (counter, key), want in known:
        assert rd.philox4x32_integers(counter, key, rounds=10) == want
        assert tuple(int(w[0]) for w in rd.philox4x32([np.array([c]) for c in counter], key, rounds=10)) == want
    rng = np.random.default_rng(5)
    counters = rng.integers(0, 2 ** 32, size=(4, 50), dtype=np.uint64)
    words = rd.philox4x32(counters, (0x9E3779B9, 0x00C0FFEE))
    for q in range(50):
        assert tuple(int(w[q]) for w in words) == rd.philox4x32_integers(counters[:, q], (0x9E3779B9, 0x00C0FFEE))


def chi_square(counts):
    expected = counts.sum() / len(counts)
    return float(((counts - expected) ** 2 / expected).sum())


def test_every_subset_of_a_small_pair_is_equally_likely():
    """s = 6, n = 2, iterations = 10: C = 15 > 10, a drawn pair.  2000 pairs give 20 000 draws over 15 subsets; chi-square
    with 14 degrees of freedom stays below its 99.9 % quantile."""
    assert rd.hypotheses(6, 2, 10) == (10, False)
    subsets = {c: q for q, c in enumerate(itertools.combinations(range(6), 2))}
    counts = np.zeros(15)
    for k in range(2000):
        for a, b in rd.drawn(UNIFORMITY_SEED, k, 6, 2, np.arange(10)):
            counts[subsets[int(a), int(b)]] += 1
    statistic = chi_square(counts)
    print("counts", counts, "chi-square", statistic)
    assert counts.sum() == 20000 and statistic < CHI2_999[14]


def test_every_row_of_a_long_pair_is_equally_likely():
    """s = 1000, n = 12: 20 000 draws (200 pairs of 100 hypotheses), the 240 000 rows counted in 100 bins of ten rows.
    The rows of one sample are distinct, which spreads them more evenly than independent ones (the variance of a bin's
    count is smaller by about (s - n) / (s - 1)), so chi-square with 99 degrees of freedom bounds the statistic from the
    safe side."""
    counts = np.zeros(100)
    repeats = 0
    for k in range(200):
        rows = rd.drawn(UNIFORMITY_SEED, k, 1000, 12, np.arange(100))
        assert (np.diff(rows, axis=1) > 0).all() and rows.min() >= 0 and rows.max() < 1000
        repeats += 100 - len({tuple(r) for r in rows.tolist()})
        counts += np.bincount(rows.reshape(-1) // 10, minlength=100)
    statistic = chi_square(counts)
    print("chi-square", statistic, "repeated samples", repeats)
    assert counts.sum() == 240000 and statistic < CHI2_999[99]
    assert repeats == 0  # (expected: H^2 / 2C = 1e4 / 2 C(1000, 12), nothing)


def test_the_new_arguments_are_refused_before_the_library(monkeypatch):
    from glimpse_amd import _lib, optimize
    from tests import ransac_pair_cases as pc

    cams, matches, d = pc.scene("kinds_px")
    call = pc.call("kinds_px", d)
    arrays = [np.arange(12)[None]] * 2
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    state = np.random.get_state()
    for change, word in (({"samples": "host"}, "samples"), ({"samples": "Device"}, "samples"), ({"samples": ""}, "samples"),
                         ({"seed": 1}, "seed"), ({"seed": 1, "samples": arrays}, "seed"), ({"seed": 0, "samples": None}, "seed"),
                         ({"samples": "device", "seed": -1}, "seed"), ({"samples": "device", "seed": 2 ** 64}, "seed"),
                         ({"samples": "device", "seed": 1.0}, "seed"), ({"samples": "device", "seed": True}, "seed"),
                         ({"samples": "device", "seed": "1"}, "seed")):
        with pytest.raises(ValueError, match=word):
            optimize.ransac_pairs(matches, **{**call, **change})
    # what the plan refuses is still refused first, and nothing above drew from np.random
    with pytest.raises(NotImplementedError, match="position"):
        optimize.ransac_pairs(matches, **{**call, "samples": "device", "seed": 1, "cam_params": {"xyz": True}})
    assert all(np.array_equal(a, b) for a, b in zip(state, np.random.get_state()))
    assert optimize.ransac_pairs({}, samples="device", seed=2 ** 64 - 1, **call) == []
