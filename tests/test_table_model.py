"""The layout model of tests/table_model.py checked against itself: its two ways of building an image agree, an image
round-trips through rows_of, check_structure accepts what build_image leaves and rejects hand-damaged images."""
import numpy as np
import pytest

from table_model import (BIT63, MAX_PROBE, U, build_image, build_image_walk, cells_of_key4, check_structure, key4_of_cells,
                         key5_of_cells, key_hash, keys_with_home, line_summaries, mix64, mix64_inv, pos_of, positions,
                         random_rows, rows_of, slot_at, sort_rows)


def mix64_int(x):
    """mix64 on one Python integer."""
    m = (1 << 64) - 1
    x = (x * 0x9E3779B97F4A7C15) & m
    x ^= x >> 29
    x = (x * 0xBF58476D1CE4E5B9) & m
    return x ^ (x >> 32)


def test_the_model_round_trips_and_rejects_damage():
    rng = np.random.default_rng(3)
    assert np.array_equal(mix64_inv(mix64(np.arange(1, 1000, dtype=U) * U(0x123456789ABCDEF))),
                          np.arange(1, 1000, dtype=U) * U(0x123456789ABCDEF))
    for x in (1, 0x1234, (1 << 64) - 1):
        assert int(mix64(np.array([x], U))[0]) == mix64_int(x)
    h = rng.integers(0, 1 << 62, size=64, dtype=np.int64).astype(U)
    for cap_log2 in (4, 7):
        every = np.stack([slot_at(h, cap_log2, p) for p in range(1 << cap_log2)], axis=1)
        assert (np.sort(every, axis=1) == np.arange(1 << cap_log2, dtype=U)).all()       # a sequence visits every slot once
        assert all(np.array_equal(pos_of(h, cap_log2, every[:, p]), np.full(64, p, U)) for p in range(1 << cap_log2))
        assert np.array_equal(every[:, 0], h & U((1 << cap_log2) - 1))
        assert (every[:, :4] >> U(2) == every[:, :1] >> U(2)).all()                      # ... its home line first
    for key_words in (1, 2):
        for cap_log2, rows in ((4, 16), (6, 40), (7, 128), (7, 1)):
            keys, q = random_rows(rng, rows, key_words)
            image = build_image(cap_log2, keys, q, key_words)
            assert np.array_equal(image, build_image_walk(cap_log2, keys, q, key_words))
            k, v = rows_of(image, key_words)
            wk, wv = sort_rows(keys, q, key_words)
            assert np.array_equal(k, wk) and np.array_equal(v.view(np.uint32), wv.view(np.uint32))
            check_structure(image, key_words, 1 << cap_log2)
        keys, q = random_rows(rng, 9000, key_words)
        image = build_image(14, keys, q, key_words)
        check_structure(image, key_words, MAX_PROBE)
        # a key given twice keeps its slot and takes the later values
        again = build_image(14, np.concatenate([keys, keys[:5]]), np.concatenate([q, q[:5] + 1]), key_words)
        assert np.array_equal(again[:, [0, 3]], image[:, [0, 3]]) and (again != image).any(axis=1).sum() == 5
        occ, pos = positions(image, key_words)
        assert pos.max() >= 1
        # damage 1: a duplicate -- a row copied into an empty slot
        hole = int(np.flatnonzero(image[:, 0] == 0)[0])
        bad = image.copy()
        bad[hole] = image[occ[0]]
        with pytest.raises(AssertionError, match="occurs again"):
            check_structure(bad, key_words, MAX_PROBE)
        # damage 2: a row behind a hole -- the slot before a displaced row, on that row's sequence, emptied
        b = int(np.flatnonzero(pos >= 1)[0])
        hb = key_hash(image[occ[b:b + 1]][:, [0, 3][:key_words]], key_words)
        bad = image.copy()
        bad[int(slot_at(hb, 14, pos[b] - 1)[0])] = 0
        with pytest.raises(AssertionError, match="is empty"):
            check_structure(bad, key_words, MAX_PROBE)
        # ... and a row too deep for the path under test
        with pytest.raises(AssertionError, match="the limit is"):
            check_structure(image, key_words, int(pos.max()))
    # damage 3: a 5x5 row with a zero second word; a key word without bit 63
    bad = image.copy()
    bad[occ[7], 3] = 0
    with pytest.raises(AssertionError, match="zero second key word"):
        check_structure(bad, 2, MAX_PROBE)
    bad = image.copy()
    bad[occ[7], 0] &= U(BIT63 - 1)
    with pytest.raises(AssertionError, match="without bit 63"):
        check_structure(bad, 2, MAX_PROBE)
    # 4x4: the spare word
    keys, q = random_rows(rng, 300, 1)
    image = build_image(10, keys, q, 1)
    summed = image.copy()
    summed[:, 3] = np.repeat(line_summaries(image, 1), 4)
    check_structure(summed, 1, MAX_PROBE, summarised=True)
    with pytest.raises(AssertionError, match="reserved"):
        check_structure(summed, 1, MAX_PROBE)
    with pytest.raises(AssertionError, match="reserved"):
        check_structure(image, 1, MAX_PROBE, summarised=True)
    assert np.array_equal(rows_of(summed, 1)[1], rows_of(image, 1)[1])
    # keys at chosen home slots; board keys
    for key_words in (1, 2):
        k = keys_with_home(rng, 26, key_words, [0, (1 << 25) - 1, 1 << 25, (1 << 26) - 1])
        assert np.array_equal(slot_at(key_hash(k, key_words), 26, 0), np.array([0, (1 << 25) - 1, 1 << 25, (1 << 26) - 1], U))
    cells = rng.integers(0, 32, size=(50, 25)).astype(np.uint8)
    k5 = key5_of_cells(cells)
    for r in range(50):
        big = sum(int(c) << (5 * i) for i, c in enumerate(cells[r]))
        assert (int(k5[r, 0]), int(k5[r, 1])) == ((big & (BIT63 - 1)) | BIT63, (big >> 63) | BIT63)
    c4 = rng.integers(0, 16, size=(50, 16)).astype(np.uint8)
    assert np.array_equal(cells_of_key4(key4_of_cells(c4)), c4)
