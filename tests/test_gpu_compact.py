"""compact_kernel alone, against numpy.

After every level of an adaptive run the kernel packs the tiles resolve_kernel left
unfrozen into the next level's active list, in their order: one block of 1024 lanes, a
ballot and mbcnt ranks inside each wave, the 16 waves' counts scanned through LDS, a
running base across rounds of 1024 entries.  The runs of test_gpu_adaptive.py hand it 9
entries - one wave of one round.  zrt_debug_compact launches it on a list of any length:

    want = list[(tile_done[list] & 0x80000000) == 0]

and every case asserts the count, the packed entries in order, and that the output past
the count still holds what the caller put there.

Sizes around a wave (64), two waves, a round (1024), a round plus a wave, two and three
rounds; keep patterns that put the kept entries in one wave, in every other lane, in every
other wave (a ballot of all ones beside a ballot of zero), nearly nowhere and nearly
everywhere; the identity list, its reverse, and a shuffled half of 2 n tiles, which reads
tile_done through the list as a run behind the scheduling probe does.

Run on an MI355X: ``pytest -m gpu``.
"""
import numpy as np
import pytest

import zraytrace_amd as z

pytestmark = pytest.mark.gpu

FROZEN = np.uint32(0x80000000)
FILL = 0xFFFFFFFF  # no tile id: a list entry is < n_tiles <= 10 000
SIZES = [1, 2, 63, 64, 65, 127, 128, 1023, 1024, 1025, 1088, 1089, 2047, 2048, 2049, 3073, 5000]
LISTS = ["identity", "reversed", "subset"]


def keep_patterns(n, rng):
    """name -> bool[n]: which list POSITIONS survive."""
    i = np.arange(n)
    one = np.zeros(n, bool)
    first, last = one.copy(), one.copy()
    first[0] = True
    last[-1] = True
    return {
        "all": np.ones(n, bool),
        "none": one,
        "first": first,
        "last": last,
        "even-entries": i % 2 == 0,
        "odd-entries": i % 2 == 1,
        "even-waves": (i // 64) % 2 == 0,
        "odd-waves": (i // 64) % 2 == 1,
        "p=0.5": rng.random(n) < 0.5,
        "p=0.02": rng.random(n) < 0.02,
        "p=0.98": rng.random(n) < 0.98,
    }


def make_list(kind, n, rng):
    """(list, n_tiles)."""
    if kind == "identity":
        return np.arange(n, dtype=np.uint32), n
    if kind == "reversed":
        return np.arange(n, dtype=np.uint32)[::-1].copy(), n
    return rng.permutation(2 * n)[:n].astype(np.uint32), 2 * n


def make_tile_done(lst, n_tiles, keep, rng):
    """resolve_kernel's words: a sample count below 2^31, bit 31 once frozen.  The tiles the
    list does not name get a random flag, so reading tile_done by position gives other answers."""
    done = rng.integers(0, 1 << 31, n_tiles, dtype=np.uint32)
    done |= np.where(rng.random(n_tiles) < 0.5, FROZEN, np.uint32(0))
    done[lst] = (done[lst] & ~FROZEN) | np.where(keep, np.uint32(0), FROZEN)
    return done


@pytest.mark.parametrize("kind", LISTS)
@pytest.mark.parametrize("n", SIZES)
def test_compact_against_numpy(n, kind):
    rng = np.random.default_rng([n, LISTS.index(kind)])
    lst, n_tiles = make_list(kind, n, rng)
    assert len(lst) == n and len(set(lst.tolist())) == n and lst.max() < n_tiles
    for name, keep in keep_patterns(n, rng).items():
        done = make_tile_done(lst, n_tiles, keep, rng)
        want = lst[(done[lst] & FROZEN) == 0]
        np.testing.assert_array_equal(want, lst[keep])  # (the inputs say what the pattern says)
        out, count = z.debug_compact(lst, done, FILL)
        where = f"n {n} list {kind} keep {name}"
        assert count == len(want), where
        np.testing.assert_array_equal(out[:count], want, err_msg=where)
        past = np.flatnonzero(out[count:] != FILL) + count
        assert past.size == 0, f"{where}: written past the count at {past[:8]}"


def test_patterns_are_what_they_claim():
    """The conditions the cases above rest on, from numpy alone: the wave patterns are whole
    ballots of ones beside whole ballots of zero, the sparse and dense patterns are neither
    empty nor full at the sizes past a round, and the sizes straddle a wave and a round."""
    rng = np.random.default_rng(0)
    pats = keep_patterns(2049, rng)
    waves = pats["even-waves"][:2048].reshape(-1, 64)
    assert waves[0::2].all() and not waves[1::2].any()
    assert 0 < pats["p=0.02"].sum() < 2049 // 10 and 2049 * 9 // 10 < pats["p=0.98"].sum() < 2049
    assert {63, 64, 65, 1023, 1024, 1025} <= set(SIZES) and max(SIZES) > 4 * 1024
