"""The bulk table kernels -- count, export, import, lookup, summaries, growth, merge -- and racing row creation, each
against the layout model of tests/table_model.py.

Tables are written and read as RAW BYTES (a uint8 [capacity, 32] tensor), so the entry point under test is the only
product code between the model and the assertion: an export is compared with rows the model read from the bytes, an
import with the bytes it left.  Every comparison is exact (integers and float32 bit patterns); there is no tolerance.
Every test runs on the CPU twin ("cpu") and on the GPU unless it says otherwise."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import table_model as M
from table_model import U
from test_table_merge import model_merge

DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
TILE = 1 << 14                                  # slots one block of the export reads per trip
CANARY_KEY, CANARY_Q = 0xA5A5A5A5A5A5A5A5, 0xDEADBEEF
TABLE_FULL, DEEP_ROW = 4, 8


# ---------------------------------------------------------------------------------------------------------------
# raw tables and the entry points, through ctypes alone
# ---------------------------------------------------------------------------------------------------------------
def lib(pkg, dev):
    return pkg._native.lib_for(torch.device(dev))


def new_table(dev, cap_log2, image=None):
    table = torch.zeros((1 << cap_log2, 32), dtype=torch.uint8, device=dev)
    if image is not None:
        write(table, image)
    return table


def write(table, image):
    table.copy_(torch.from_numpy(np.ascontiguousarray(image).view(np.uint8).reshape(-1, 32)))


def raw(table):
    return table.cpu().numpy().view(U).reshape(-1, 4).copy()


def i64(dev, *values):
    return torch.tensor(values, dtype=torch.int64, device=dev)


def count(L, dev, table, cap_log2, start=0):
    c = i64(dev, start)
    assert L.q2048_table_count(table.data_ptr(), cap_log2, c.data_ptr(), None) == 0
    return int(c.item())


def canary_buffers(dev, room, key_words):
    keys = torch.full((room, key_words), CANARY_KEY - (1 << 64), dtype=torch.int64, device=dev)
    q = torch.full((room, 4), CANARY_Q - (1 << 32), dtype=torch.int32, device=dev)
    return keys, q


def export(L, dev, table, cap_log2, key_words, max_rows, start=0, room=None, bufs=None):
    """q2048_table_export into buffers of `room` records pre-filled with a canary.  Returns (keys uint64 [room, words],
    q as uint32 bit patterns [room, 4], *count afterwards, the buffers)."""
    room = max(max_rows, start) + 64 if room is None else room
    keys, q = canary_buffers(dev, room, key_words) if bufs is None else bufs
    c = i64(dev, start)
    assert L.q2048_table_export(table.data_ptr(), cap_log2, keys.data_ptr(), q.data_ptr(), max_rows, key_words,
                                c.data_ptr(), None) == 0
    return keys.cpu().numpy().view(U), q.cpu().numpy().view(np.uint32), int(c.item()), (keys, q)


def untouched(keys, qbits):
    return (keys == U(CANARY_KEY)).all(axis=1) & (qbits == np.uint32(CANARY_Q)).all(axis=1)


def assert_same_rows(got_keys, got_qbits, want, key_words, what=""):
    """Exported records against the model's (keys, q) sorted by key: the same rows, bit for bit."""
    gk, gq = M.sort_rows(got_keys, got_qbits.view(np.float32), key_words)
    wk, wq = want
    assert len(gk) == len(wk), f"{what}: {len(gk)} rows, the model has {len(wk)}"
    assert np.array_equal(gk, wk), f"{what}: key sets differ, first at row {np.argwhere(gk != wk)[0]} by key order"
    bad = gq.view(np.uint32) != wq.view(np.uint32)
    assert not bad.any(), f"{what}: values differ, first at {np.argwhere(bad)[0]}"


def do_import(L, dev, table, cap_log2, keys, q, key_words):
    tk = torch.from_numpy(M.keys2d(keys, key_words).view(np.int64)).to(dev)
    tq = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    assert L.q2048_table_import(table.data_ptr(), cap_log2, tk.data_ptr(), tq.data_ptr(), len(tq), key_words,
                                st.data_ptr(), None) == 0
    return int(st.item())


def deep_rows(image, key_words):
    """Does the image hold a row beyond the learning paths' probe limit?"""
    _, pos = M.positions(image, key_words)
    return bool((pos >= min(M.ROLLOUT_PROBE, len(image))).any())


# ---------------------------------------------------------------------------------------------------------------
# images, built once and shared
# ---------------------------------------------------------------------------------------------------------------
_IMAGES = {}
LOADS = ["empty", "one", "half", "full"]


def edge_slots(cap_log2):
    """The slots a tiling is most likely to lose: the table's first and last, and those either side of a tile border."""
    cap = 1 << cap_log2
    return sorted({0, cap - 1} | ({TILE - 1, TILE} if cap > TILE else set()))


def image_of(cap_log2, load, key_words):
    """(image, rows of the image by the model) for one capacity and load.  `one`: the table's last slot.  `half`: the
    edge slots first -- each by a key whose home it is -- then random keys to load 0.5.  `full`: every slot."""
    key = (cap_log2, load, key_words)
    if key not in _IMAGES:
        rng = np.random.default_rng(1000 * cap_log2 + 10 * LOADS.index(load) + key_words)
        cap = 1 << cap_log2
        if load == "empty":
            keys, q = M.random_rows(rng, 0, key_words)
        elif load == "one":
            keys, q = M.keys_with_home(rng, cap_log2, key_words, [cap - 1]), rng.standard_normal((1, 4)).astype(np.float32)
        else:
            edge = M.keys2d(M.keys_with_home(rng, cap_log2, key_words, edge_slots(cap_log2)), key_words)
            rows = cap if load == "full" else cap // 2
            more, q = M.random_rows(rng, rows, key_words)
            keys = np.concatenate([edge, M.keys2d(more, key_words)])[:rows]
            assert len(np.unique(keys, axis=0)) == rows
        image = M.build_image(cap_log2, keys, q, key_words)
        occupied = np.flatnonzero(image[:, 0] != 0)
        assert len(occupied) == len(q)
        if load in ("half", "full"):
            assert set(edge_slots(cap_log2)) <= set(occupied.tolist())
        if load == "one":
            assert occupied.tolist() == [cap - 1]
        M.check_structure(image, key_words, cap)
        _IMAGES[key] = (image, M.rows_of(image, key_words))
    return _IMAGES[key]


def filled(cap_log2, load, key_words, seed):
    """A random image at a fractional load: (image, keys in insertion order, q)."""
    key = ("filled", cap_log2, load, key_words, seed)
    if key not in _IMAGES:
        rng = np.random.default_rng(seed)
        keys, q = M.random_rows(rng, int(load * (1 << cap_log2)), key_words)
        _IMAGES[key] = (M.build_image(cap_log2, keys, q, key_words), keys, q)
    return _IMAGES[key]


# ---------------------------------------------------------------------------------------------------------------
# 1. count and export on a host-written image
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("load", LOADS)
@pytest.mark.parametrize("cap_log2", [4, 13, 14, 15])
def test_count_and_export_of_a_written_image(pkg, dev, n, load, cap_log2):
    """16 slots (less than a block's first load row), half a tile, exactly one tile, two tiles / two blocks; empty, one
    row in the last slot, load 0.5 with the edge slots occupied, completely full."""
    L, words = lib(pkg, dev), 1 if n == 4 else 2
    image, want = image_of(cap_log2, load, words)
    rows = len(want[0])
    table = new_table(dev, cap_log2, image)
    assert count(L, dev, table, cap_log2) == rows
    keys, qbits, c, _ = export(L, dev, table, cap_log2, words, rows)
    assert c == rows
    assert_same_rows(keys[:rows], qbits[:rows], want, words, f"2^{cap_log2} {load}")
    assert untouched(keys[rows:], qbits[rows:]).all(), "records written beyond the rows"
    assert np.array_equal(raw(table), image), "a read-only pass wrote the table"
    if n == 4 and rows:
        # a summarised 4x4 table: the spare words hold summaries, which are no part of a key or a value
        summed = image.copy()
        summed[:, 3] = np.repeat(M.line_summaries(image, 1), 4)
        assert (summed[:, 3] != 0).any()
        write(table, summed)
        assert count(L, dev, table, cap_log2) == rows
        keys, qbits, c, _ = export(L, dev, table, cap_log2, 1, rows)
        assert c == rows
        assert_same_rows(keys[:rows], qbits[:rows], want, 1, f"2^{cap_log2} {load}, summarised")


# ---------------------------------------------------------------------------------------------------------------
# 2. the grid-stride second trip (GPU: the grids are capped at 2048 and 8192 blocks)
# ---------------------------------------------------------------------------------------------------------------
def scattered_rows(rng, cap_log2, key_words, rows, must):
    """`rows` random rows, each at its key's home slot (model-placed; rows whose home is taken already are left out),
    among them one at every slot of `must`.  -> (slots int64 [R], words uint64 [R, 4])"""
    keys, q = M.random_rows(rng, rows, key_words)
    keys = np.concatenate([M.keys2d(M.keys_with_home(rng, cap_log2, key_words, must), key_words), M.keys2d(keys, key_words)])
    q = np.concatenate([rng.standard_normal((len(must), 4)).astype(np.float32), q])
    slots = M.slot_at(M.key_hash(keys, key_words), cap_log2, 0).astype(np.int64)
    _, first = np.unique(slots, return_index=True)
    first = np.sort(first)
    assert set(must) <= set(slots[first].tolist())
    return slots[first], M.slot_words(keys[first], q[first], key_words), keys[first], q[first]


def scatter(table, slots, words):
    table.view(torch.int64).reshape(-1, 4)[torch.from_numpy(slots).to(table.device)] = \
        torch.from_numpy(words.view(np.int64)).to(table.device)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5])
def test_export_second_grid_stride_trip(pkg, n):
    """A 2^26-slot table is 4096 tiles for at most 2048 blocks: every block makes a second trip.  A few thousand rows at
    their home slots, among them the last slot of the first trip, the first of the second and the table's last."""
    dev, cap_log2, words = "cuda:0", 26, 1 if n == 4 else 2
    L = lib(pkg, dev)
    rng = np.random.default_rng(26 + n)
    must = [0, TILE - 1, TILE, (1 << 25) - 1, 1 << 25, (1 << 25) + TILE, (1 << 26) - 1]
    slots, slot_w, keys, q = scattered_rows(rng, cap_log2, words, 3000, must)
    table = new_table(dev, cap_log2)
    scatter(table, slots, slot_w)
    rows = len(slots)
    assert count(L, dev, table, cap_log2) == rows
    got_k, got_q, c, _ = export(L, dev, table, cap_log2, words, rows)
    assert c == rows
    assert_same_rows(got_k[:rows], got_q[:rows], M.sort_rows(keys, q, words), words, "2^26 slots")
    assert untouched(got_k[rows:], got_q[rows:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5])
def test_summaries_second_grid_stride_trip(pkg, n):
    """2^24 slots are 2^22 lines, twice what 8192 blocks of 256 lanes cover in one trip.  Every non-zero summary word
    must be the model's word of a line that holds rows, and every such line must have its word: so every other line,
    not just a sample, reads as zero."""
    dev, cap_log2, words = "cuda:0", 24, 1 if n == 4 else 2
    L = lib(pkg, dev)
    rng = np.random.default_rng(24 + n)
    half = 1 << 23                                                   # slots of the first trip
    must = [0, 3, half - 4, half - 1, half, half + 5, (1 << 24) - 4, (1 << 24) - 1]
    slots, slot_w, keys, q = scattered_rows(rng, cap_log2, words, 3000, must)
    table = new_table(dev, cap_log2)
    scatter(table, slots, slot_w)
    want_lines, want_words = M.summary_words(slots, M.key_hash(keys, words))
    before = table.clone()
    side = torch.full((1 << 22,), 0x5555, dtype=torch.int64, device=dev)
    assert L.q2048_table_summarise_side(table.data_ptr(), cap_log2, words, side.data_ptr(), None) == 0
    at = torch.nonzero(side).reshape(-1)
    assert np.array_equal(at.cpu().numpy(), want_lines.astype(np.int64))
    assert np.array_equal(side[at].cpu().numpy().view(U), want_words)
    assert torch.equal(table, before), "the side pass wrote the table"
    del before
    if n == 4:
        assert L.q2048_table_summarise(table.data_ptr(), cap_log2, None) == 0
        t = table.view(torch.int64).reshape(-1, 4)
        at = torch.nonzero(t[:, 3]).reshape(-1)
        want_slots = (want_lines.astype(np.int64)[:, None] * 4 + np.arange(4)[None, :]).reshape(-1)
        assert np.array_equal(at.cpu().numpy(), want_slots)
        assert np.array_equal(t[at, 3].cpu().numpy().view(U), np.repeat(want_words, 4))
        # the pass writes the spare words and nothing else
        t[:, 3] = 0
        occupied = torch.nonzero(t[:, 0]).reshape(-1)
        assert np.array_equal(occupied.cpu().numpy(), np.sort(slots))
        assert np.array_equal(t[torch.from_numpy(slots).to(dev)].cpu().numpy().view(U), slot_w)


# ---------------------------------------------------------------------------------------------------------------
# 3. truncation and the cursor
# ---------------------------------------------------------------------------------------------------------------
def assert_records_are_rows(keys, qbits, want, key_words, what):
    """Every record is a row of the table with its own values, and no row comes twice."""
    k = M.keys2d(keys, key_words)
    assert len(np.unique(k, axis=0)) == len(k), f"{what}: a row was exported twice"
    wk, wq = want
    both = np.concatenate([wk, k])
    u, inv = np.unique(both, axis=0, return_inverse=True)
    assert len(u) == len(wk), f"{what}: a record is no row of the table"
    pos = inv.reshape(-1)[len(wk):]
    assert np.array_equal(wq.view(np.uint32)[pos], qbits), f"{what}: a record carries another row's values"


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("cap_log2", [13, 16])
def test_export_truncates_at_max_rows(pkg, dev, n, cap_log2):
    """max_rows = 0, 1, rows - 1, rows, rows + 1: *count is the number of occupied slots every time, exactly
    min(rows, max_rows) records are written, all of them distinct rows of the table, and nothing beyond max_rows is
    touched.  2^16 slots at load 0.5 are four tiles: four blocks race for their ranges."""
    L, words = lib(pkg, dev), 1 if n == 4 else 2
    image, _, _ = filled(cap_log2, 0.5, words, seed=31 + n)
    want = M.rows_of(image, words)
    rows = len(want[0])
    table = new_table(dev, cap_log2, image)
    for max_rows in (0, 1, rows - 1, rows, rows + 1):
        keys, qbits, c, _ = export(L, dev, table, cap_log2, words, max_rows, room=rows + 64)
        assert c == rows, f"max_rows={max_rows}: *count = {c}, the table holds {rows}"
        wrote = min(rows, max_rows)
        clean = untouched(keys, qbits)
        assert clean[wrote:].all(), f"max_rows={max_rows}: record {wrote + int(np.argmin(clean[wrote:]))} was written"
        assert not (keys[:wrote] == U(CANARY_KEY)).all(axis=1).any(), f"max_rows={max_rows}: a record below it was not written"
        assert_records_are_rows(keys[:wrote], qbits[:wrote], want, words, f"max_rows={max_rows}")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_export_appends_at_the_cursor(pkg, dev, n):
    """*count is the export's write cursor (include/q2048.h): records go to [count0, ...) below max_rows and *count ends
    at count0 + occupied.  Two tables exported one after the other with one cursor give the union of their rows.
    q2048_table_count is a plain addition."""
    L, words = lib(pkg, dev), 1 if n == 4 else 2
    img_a, _, _ = filled(15, 0.4, words, seed=41 + n)
    img_b, _, _ = filled(13, 0.7, words, seed=43 + n)
    a, b = M.rows_of(img_a, words), M.rows_of(img_b, words)
    ra, rb = len(a[0]), len(b[0])
    ta, tb = new_table(dev, 15, img_a), new_table(dev, 13, img_b)
    assert count(L, dev, ta, 15, start=1000) == 1000 + ra
    assert count(L, dev, tb, 13, start=-5) == rb - 5
    start, room = 37, 37 + ra + rb + 64
    # all of A behind the cursor
    keys, qbits, c, bufs = export(L, dev, ta, 15, words, start + ra, start=start, room=room)
    assert c == start + ra
    clean = untouched(keys, qbits)
    assert clean[:start].all() and clean[start + ra:].all(), "records outside [count0, count0 + rows)"
    assert_same_rows(keys[start:c], qbits[start:c], a, words, "behind the cursor")
    # ... then B into the same buffers with the same cursor: the union
    keys, qbits, c2, _ = export(L, dev, tb, 13, words, room, start=c, room=room, bufs=bufs)
    assert c2 == start + ra + rb
    clean = untouched(keys, qbits)
    assert clean[:start].all() and clean[c2:].all()
    union = M.sort_rows(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]), words)
    assert_same_rows(keys[start:c2], qbits[start:c2], union, words, "two tables, one cursor")
    # bounded by max_rows, which is an index into the buffers, not a number of rows of this call
    keys, qbits, c, _ = export(L, dev, ta, 15, words, start + ra // 2, start=start, room=room)
    assert c == start + ra
    clean = untouched(keys, qbits)
    assert clean[:start].all() and clean[start + ra // 2:].all() and not clean[start:start + ra // 2].any()
    assert_records_are_rows(keys[start:start + ra // 2], qbits[start:start + ra // 2], a, words, "cursor and max_rows")
    # a cursor at or beyond max_rows: everything is counted, nothing written
    keys, qbits, c, _ = export(L, dev, ta, 15, words, start, start=start + 3, room=room)
    assert c == start + 3 + ra and untouched(keys, qbits).all()


# ---------------------------------------------------------------------------------------------------------------
# 4. import
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("load", [0.5, 0.93, 0.99])
def test_import_leaves_a_sound_table(pkg, dev, n, load):
    """Random rows into an empty 2^14-slot table: the bytes hold exactly the input, every row where a probe finds it.
    DEEP_ROW is raised exactly when a row lies beyond the learning paths' 2^10 positions (never at load 0.5)."""
    L, words, cap_log2 = lib(pkg, dev), 1 if n == 4 else 2, 14
    rng = np.random.default_rng(int(load * 100) + n)
    keys, q = M.random_rows(rng, int(load * (1 << cap_log2)), words)
    table = new_table(dev, cap_log2)
    status = do_import(L, dev, table, cap_log2, keys, q, words)
    image = raw(table)
    got, want = M.rows_of(image, words), M.sort_rows(keys, q, words)
    assert len(got[0]) == len(want[0]), f"{len(got[0])} rows in the table, {len(want[0])} imported"
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    M.check_structure(image, words, M.MAX_PROBE)
    assert status == (DEEP_ROW if deep_rows(image, words) else 0)
    if load == 0.5:
        assert status == 0
    # the same keys with new values: overwritten in place -- the image changes in the value words only
    q2 = rng.standard_normal(q.shape).astype(np.float32)
    status = do_import(L, dev, table, cap_log2, keys, q2, words)
    again = raw(table)
    assert np.array_equal(again[:, [0, 3]], image[:, [0, 3]]), "a re-import moved or created a key word"
    got = M.rows_of(again, words)
    assert np.array_equal(got[1].view(np.uint32), M.sort_rows(keys, q2, words)[1].view(np.uint32))
    assert status == (DEEP_ROW if deep_rows(image, words) else 0)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_import_into_a_table_that_is_too_small(pkg, dev, n):
    L, words, cap_log2 = lib(pkg, dev), 1 if n == 4 else 2, 4
    keys, q = M.random_rows(np.random.default_rng(50 + n), 24, words)
    table = new_table(dev, cap_log2)
    status = do_import(L, dev, table, cap_log2, keys, q, words)
    assert status & TABLE_FULL and not status & ~(TABLE_FULL | DEEP_ROW)
    image = raw(table)
    got = M.rows_of(image, words)
    assert len(got[0]) == 16
    assert_records_are_rows(got[0], got[1].view(np.uint32), M.sort_rows(keys, q, words), words, "a full table")
    M.check_structure(image, words, M.MAX_PROBE)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_import_of_one_key_several_times(pkg, dev, n):
    """include/q2048.h: a key given more than once in one call leaves ONE row, and each of its four values is that
    component of one of the duplicates."""
    L, words, cap_log2 = lib(pkg, dev), 1 if n == 4 else 2, 10
    rng = np.random.default_rng(60 + n)
    keys, _ = M.random_rows(rng, 300, words)
    keys = M.keys2d(keys, words)
    idx = np.repeat(np.arange(299), np.concatenate([np.full(100, 1), np.full(150, 2), np.full(49, 3)]))
    rng.shuffle(idx)
    idx = np.concatenate([idx[:192], np.full(64, 299), idx[192:]])   # the last key 64 times in a row: one whole wave
    q = rng.standard_normal((len(idx), 4)).astype(np.float32)
    table = new_table(dev, cap_log2)
    assert do_import(L, dev, table, cap_log2, keys[idx], q, words) == 0
    image = raw(table)
    M.check_structure(image, words, M.MAX_PROBE)
    gk, gq = M.rows_of(image, words)
    order = np.lexsort(keys.T[::-1])
    assert np.array_equal(gk, keys[order]), "one row per key"
    for r, k in enumerate(order):
        given = q[idx == k].view(np.uint32)
        for a in range(4):
            assert gq.view(np.uint32)[r, a] in given[:, a], f"key {k}, action {a}: a value none of the duplicates gave"


# ---------------------------------------------------------------------------------------------------------------
# 5. lookup on a host-written image
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_lookup_on_a_written_image(pkg, dev, n):
    """q2048_q_lookup (2^14 positions) on a table the library did not build: load 0.93, written by the model.  Present
    boards return their rows, absent boards zeros and found = 0."""
    L, words, cap_log2 = lib(pkg, dev), 1 if n == 4 else 2, 14
    rng = np.random.default_rng(70 + n)
    rows = int(0.93 * (1 << cap_log2))
    if n == 4:
        keys, _ = M.random_rows(rng, rows + 500, 1)
        cells = M.cells_of_key4(keys)
        assert np.array_equal(M.key4_of_cells(cells), keys)
    else:
        cells = np.unique(rng.integers(0, 32, size=(rows + 600, 25)).astype(np.uint8), axis=0)
        rng.shuffle(cells)
        cells = cells[:rows + 500]
        keys = M.key5_of_cells(cells)
    q = rng.standard_normal((rows, 4)).astype(np.float32)
    image = M.build_image(cap_log2, keys[:rows], q, words)
    M.check_structure(image, words, M.MAX_PROBE)
    _, pos = M.positions(image, words)
    assert pos.max() > 64                                            # rows many lines away from their home
    table = new_table(dev, cap_log2, image)
    boards = torch.from_numpy(cells).to(dev)
    out = torch.full((len(cells), 4), 7.0, dtype=torch.float32, device=dev)
    found = torch.full((len(cells),), 9, dtype=torch.uint8, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    assert L.q2048_q_lookup(table.data_ptr(), cap_log2, boards.data_ptr(), len(cells), n, 0, 0, out.data_ptr(),
                            found.data_ptr(), st.data_ptr(), None) == 0
    out, found = out.cpu().numpy(), found.cpu().numpy()
    assert int(st.item()) == 0
    assert (found[:rows] == 1).all(), f"{int((found[:rows] != 1).sum())} present rows not found, first {int(np.argmax(found[:rows] != 1))}"
    assert np.array_equal(out[:rows].view(np.uint32), q.view(np.uint32))
    assert (found[rows:] == 0).all() and (out[rows:].view(np.uint32) == 0).all()
    assert np.array_equal(raw(table), image)


# ---------------------------------------------------------------------------------------------------------------
# 6. growth (the chunk allocator has no host form)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n,summarised", [(4, False), (4, True), (5, False)])
def test_growth_moves_every_row(pkg, n, summarised):
    """q2048_table_grow 2^14 -> 2^16 on a table imported to load 0.9: the new table's bytes hold the old table's rows,
    every one where a probe finds it; a summarised 4x4 table leaves no summary word behind."""
    dev, words = torch.device("cuda:0"), 1 if n == 4 else 2
    L = lib(pkg, dev)
    chunked = importlib.import_module(pkg.__name__ + ".agent")._ChunkedTable
    keys, q = M.random_rows(np.random.default_rng(80 + n), int(0.9 * (1 << 14)), words)
    owner = chunked(14, dev, max_capacity_log2=16)
    table = owner.tensor(dev)
    status = do_import(L, dev, table, 14, keys, q, words)
    if summarised:
        assert L.q2048_table_summarise(table.data_ptr(), 14, None) == 0
    old = raw(table)
    assert status == (DEEP_ROW if deep_rows(old, words) else 0)
    M.check_structure(old, words, M.MAX_PROBE, summarised=summarised)
    del table
    torch.cuda.synchronize()
    bigger, moved = owner.grow(16, words, None)
    new = raw(bigger.tensor(dev))
    want, got = M.rows_of(old, words), M.rows_of(new, words)
    assert moved == len(want[0]) == len(q)
    assert len(got[0]) == len(want[0])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    M.check_structure(new, words, M.MAX_PROBE)                       # (4x4: every `reserved` word is 0)


# ---------------------------------------------------------------------------------------------------------------
# 7. merge, on raw bytes
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("mode,w", [("add", 0.25), ("blend", 0.3)])
def test_merge_on_raw_bytes(pkg, dev, n, mode, w):
    """A 2^16-slot source into a 2^14-slot destination that ends near load 0.9, both written by the model; the expected
    rows are test_table_merge's model fed from the raw bytes."""
    L, words = lib(pkg, dev), 1 if n == 4 else 2
    rng = np.random.default_rng(90 + n)
    keys, _ = M.random_rows(rng, 14700, words)                       # 14700 / 16384 = 0.897
    keys = M.keys2d(keys, words)
    dst_keys, src_keys = keys[:8000], keys[6000:]                    # 2000 shared, 6700 only in the source
    dst_img = M.build_image(14, dst_keys, rng.standard_normal((8000, 4)).astype(np.float32), words)
    src_img = M.build_image(16, src_keys, rng.standard_normal((8700, 4)).astype(np.float32), words)
    if n == 4:                                                       # a summarised source: its spare words are not rows
        src_img[:, 3] = np.repeat(M.line_summaries(src_img, 1), 4)
    dst, src = new_table(dev, 14, dst_img), new_table(dev, 16, src_img)
    mk, mq, created, combined = model_merge(M.rows_of(dst_img, words), M.rows_of(src_img, words), mode, w)
    assert (created, combined) == (6700, 2000)
    counters, st = i64(dev, 0, 0, 0, 0), torch.zeros(1, dtype=torch.int32, device=dev)
    assert L.q2048_table_merge(dst.data_ptr(), 14, src.data_ptr(), 16, words, 0 if mode == "add" else 1, w,
                               counters.data_ptr(), st.data_ptr(), None) == 0
    assert counters.tolist() == [8700, created, combined, 0]
    after = raw(dst)
    assert np.array_equal(raw(src), src_img), "the source was written"
    M.check_structure(after, words, M.MAX_PROBE)                     # (4x4: no summary word reached dst)
    got = M.rows_of(after, words)
    assert len(got[0]) == len(mk)
    assert np.array_equal(got[0], mk.reshape(got[0].shape)), "key sets differ"
    bad = got[1].view(np.uint32) != np.ascontiguousarray(mq).view(np.uint32)
    assert not bad.any(), f"{int(bad.any(axis=1).sum())} rows differ in their bits, first at {np.argwhere(bad)[0]}"
    # rows that were there stay where they were
    there = dst_img[:, 0] != 0
    assert np.array_equal(after[there][:, [0, 3]], dst_img[there][:, [0, 3]])
    _, pos = M.positions(after, words)
    new_deep = bool((pos[~there[np.flatnonzero(after[:, 0] != 0)]] >= M.ROLLOUT_PROBE).any())
    assert int(st.item()) == (DEEP_ROW if new_deep else 0)


# ---------------------------------------------------------------------------------------------------------------
# 8. racing creation
# ---------------------------------------------------------------------------------------------------------------
RACE_B, RACE_SEED = 4096, 5
_TWIN_KEYS = {}


def race_pair(pkg, dev, n, cap_log2):
    env = pkg.BatchedGame2048Env(RACE_B, board_size=n, seed=RACE_SEED, env_id0=0, device=dev)
    agent = pkg.BatchedQLearningAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=1.0,
                                      capacity_log2=cap_log2, seed=RACE_SEED, env_id0=0, device=dev, board_size=n,
                                      freeze_load=None)
    assert agent.epsilon == 1.0
    return env, agent


def twin_keys(pkg, n, steps):
    """The states `steps` steps of uniformly random play visit (epsilon = 1: the actions are the draws', whatever the
    table holds), from a fused rollout of the CPU twin into a table large enough to hold them all: sorted keys."""
    if (n, steps) not in _TWIN_KEYS:
        env, agent = race_pair(pkg, "cpu", n, 20)
        agent.fused_rollout(env, steps)
        assert agent.check_status() == 0 and agent.stats()["drops"] == 0
        _TWIN_KEYS[(n, steps)] = M.rows_of(raw(agent.table), 1 if n == 4 else 2)[0]
    return _TWIN_KEYS[(n, steps)]


def assert_race_left_a_sound_table(pkg, agent, n, want_keys, full=False):
    if agent.on_gpu:
        torch.cuda.synchronize()
    words = 1 if n == 4 else 2
    image = raw(agent.table)
    M.check_structure(image, words, M.ROLLOUT_PROBE)
    stats, status = agent.stats(), agent.check_status()
    got = M.rows_of(image, words)[0]
    assert len(got) == stats["inserts"], f"{len(got)} occupied slots, {stats['inserts']} rows created by the counters"
    assert pkg._native.claim_timeouts(agent._L) == 0
    if not full:
        assert status == 0 and stats["drops"] == 0
        assert len(got) == len(want_keys) and np.array_equal(got, want_keys), "the key set differs from the CPU twin's"
    else:
        # the workload visits more states than the table has slots: it fills up, and what it holds are states visited
        assert status == TABLE_FULL and stats["drops"] > 0 and len(want_keys) > len(image)
        assert len(got) > 0.97 * len(image)
        assert len(np.unique(np.concatenate([want_keys, got]), axis=0)) == len(want_keys), "a key no env ever visited"


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("cap_log2", [16, 19])
def test_rows_created_by_a_racing_fused_rollout(pkg, dev, n, cap_log2):
    """4096 envs of a shared table, epsilon = 1, 64 steps in one launch.  The workload visits 217 595 (4x4) / 236 251
    (5x5) states.  2^19 slots hold them at load 0.42 / 0.45: nothing is dropped and the key set is the twin's.  2^16 slots
    do not: there the table must fill up soundly -- same structure, same counters' identity, TABLE_FULL and nothing
    else, only keys of visited states."""
    env, agent = race_pair(pkg, dev, n, cap_log2)
    agent.fused_rollout(env, 64)
    assert_race_left_a_sound_table(pkg, agent, n, twin_keys(pkg, n, 64), full=cap_log2 == 16)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_rows_created_by_the_racing_four_call_loop(pkg, dev, n):
    """The same workload through choose / step / update / reset, 16 steps into 2^16 slots (load 0.70 / 0.83)."""
    env, agent = race_pair(pkg, dev, n, 16)
    s = env.boards
    for _ in range(16):
        a = agent.choose_action(s)
        s2, r, d, _ = env.step(a)
        agent.update_q_value(s, a, r, s2, d)
        s = env.reset(d)
    assert_race_left_a_sound_table(pkg, agent, n, twin_keys(pkg, n, 16))


def test_abi_version_is_unchanged(pkg):
    assert pkg._native.host_lib().q2048_abi_version() == 7
    assert C.CDLL(pkg._native.LIB_PATH).q2048_abi_version() == 7     # (loads without a GPU: no compute call)
