"""An independent model of the Q-table's memory layout: pure Python and numpy on uint64 arrays, restated from
include/q2048.h and the comments of csrc/q2048_kernels.hip.  It shares no code with the product, so a table's RAW BYTES
can be judged without going through the table's own bulk kernels (count, export, import), which is what
tests/test_table_kernels.py does.

The layout
  slot      four little-endian 64-bit words: [0] key, [1] q0 | q1 << 32, [2] q2 | q3 << 32 (float32 bit patterns),
            [3] `reserved` -- 4x4: 0, or the line's summary word once the table is summarised; 5x5: the second key word.
            A slot is occupied when word 0 is not 0.  5x5 key words both carry bit 63.
  hash      4x4: mix64(key); 5x5: mix64(key ^ second * 0x9E3779B97F4A7C15).
  sequence  bucketised: four slots are one 128-byte line.  The sequence of a key starts at its home slot hash & mask,
            visits the other three slots of that line cyclically, then moves to the next line and visits it in the same
            order: position p is slot ((line0 + p // 4) & line_mask) * 4 + ((hash + p) & 3).  Positions 0 .. capacity-1
            visit every slot exactly once.
  invariant there is no deletion, so no empty slot lies before a row on that row's own sequence, and no key occurs twice.
  summary   one 64-bit word per line: bits 16r .. 16r+15 are 0 when slot r of the line is empty, else
            ((hash >> 48) & 0xffff) | 1.

A table image here is a uint64 array [2^cap_log2, 4]; `image.view(np.uint8).reshape(-1, 32)` are the table's bytes."""
import numpy as np

U = np.uint64
GOLDEN = 0x9E3779B97F4A7C15
MIX2 = 0xBF58476D1CE4E5B9
BIT63 = 1 << 63
_M64 = (1 << 64) - 1
MAX_PROBE = 1 << 14        # import, growth, merge, q2048_q_lookup (kMaxProbe), or the whole table when it is smaller
ROLLOUT_PROBE = 1 << 10    # rows created by rollouts, choose and update (kRolloutProbe)


def mix64(x):
    """The table's 64-bit mixer on uint64 arrays (wraps modulo 2^64)."""
    x = np.asarray(x, dtype=U).copy()
    with np.errstate(over="ignore"):
        x *= U(GOLDEN)
        x ^= x >> U(29)
        x *= U(MIX2)
        x ^= x >> U(32)
    return x


def mix64_inv(h):
    """Inverse of mix64 (every step is a bijection of 64-bit words): the key with a given hash, used to put a row at a
    chosen home slot."""
    h = np.asarray(h, dtype=U).copy()
    with np.errstate(over="ignore"):
        h ^= h >> U(32)
        h *= U(pow(MIX2, -1, 1 << 64))
        h ^= (h >> U(29)) ^ (h >> U(58))
        h *= U(pow(GOLDEN, -1, 1 << 64))
    return h


def keys2d(keys, key_words):
    k = np.ascontiguousarray(keys, dtype=U)
    return k.reshape(-1, key_words)


def key_hash(keys, key_words):
    """keys: uint64 [R] or [R, key_words] -> hash uint64 [R]."""
    k = keys2d(keys, key_words)
    if key_words == 1:
        return mix64(k[:, 0])
    with np.errstate(over="ignore"):
        return mix64(k[:, 0] ^ (k[:, 1] * U(GOLDEN)))


def slot_at(hash, cap_log2, p):
    """Slot at position p of the sequence of a key with this hash."""
    hash, p = np.asarray(hash, dtype=U), np.asarray(p, dtype=U)
    mask = U((1 << cap_log2) - 1)
    line0, lmask, off = (hash & mask) >> U(2), mask >> U(2), hash & U(3)
    return (((line0 + (p >> U(2))) & lmask) << U(2)) | ((off + p) & U(3))


def pos_of(hash, cap_log2, slot):
    """Position of `slot` on the sequence of a key with this hash (the inverse of slot_at)."""
    hash, slot = np.asarray(hash, dtype=U), np.asarray(slot, dtype=U)
    mask = U((1 << cap_log2) - 1)
    line0, lmask, off = (hash & mask) >> U(2), mask >> U(2), hash & U(3)
    with np.errstate(over="ignore"):
        return ((((slot >> U(2)) - line0) & lmask) << U(2)) | ((slot - off) & U(3))


def fingerprint(hash):
    """The 16-bit fingerprint a line's summary word carries for an occupied slot (never 0)."""
    return ((np.asarray(hash, dtype=U) >> U(48)) & U(0xFFFF)) | U(1)


def summary_words(slots, hashes):
    """The summary words of the lines that hold rows at `slots` (keys hashing to `hashes`): (lines sorted, words)."""
    slots, hashes = np.asarray(slots, dtype=U), np.asarray(hashes, dtype=U)
    lines, inv = np.unique(slots >> U(2), return_inverse=True)
    words = np.zeros(len(lines), U)
    np.bitwise_or.at(words, inv, fingerprint(hashes) << (U(16) * (slots & U(3))))
    return lines, words


def line_summaries(image, key_words):
    """The summary word of every line of an image: uint64 [capacity / 4]."""
    occ = np.flatnonzero(image[:, 0] != 0)
    out = np.zeros(len(image) >> 2, U)
    if len(occ):
        lines, words = summary_words(occ, key_hash(image[occ][:, [0, 3][:key_words]], key_words))
        out[lines.astype(np.int64)] = words
    return out


def key5_of_cells(cells):
    """The two key words of 5x5 boards: cells uint8 [R, 25] of 5-bit log2 tiles, cell c in bits 5c .. 5c+4 of a 125-bit
    number; word 0 = bits 0..62 | bit 63, word 1 = bits 63..124 | bit 63."""
    c = np.asarray(cells, dtype=U).reshape(-1, 25)
    assert (c < U(32)).all()
    lo, hi = np.zeros(len(c), U), np.zeros(len(c), U)
    for i in range(25):
        if 5 * i + 5 <= 63:
            lo |= c[:, i] << U(5 * i)
        elif 5 * i >= 63:
            hi |= c[:, i] << U(5 * i - 63)
        else:                                                    # cell 12 lies across the two words: bits 60..64
            lo |= (c[:, i] << U(5 * i)) & U(BIT63 - 1)
            hi |= c[:, i] >> U(63 - 5 * i)
    return np.stack([lo | U(BIT63), hi | U(BIT63)], axis=1)


def key4_of_cells(cells):
    """The key of 4x4 boards: cells uint8 [R, 16] of log2 tiles 0..15, cell 0 in the low nibble."""
    c = np.asarray(cells, dtype=U).reshape(-1, 16)
    assert (c < U(16)).all()
    k = np.zeros(len(c), U)
    for i in range(16):
        k |= c[:, i] << U(4 * i)
    return k


def cells_of_key4(keys):
    k = np.asarray(keys, dtype=U).reshape(-1)
    return np.stack([((k >> U(4 * c)) & U(15)).astype(np.uint8) for c in range(16)], axis=1)


def keys_with_home(rng, cap_log2, key_words, slots):
    """One key per entry of `slots` whose home slot (position 0 of its sequence) is that slot; distinct hashes."""
    slots = np.asarray(slots, dtype=U)
    mask = U((1 << cap_log2) - 1)
    out = np.zeros((len(slots), key_words), U)
    todo = np.arange(len(slots))
    while len(todo):
        h = (rng.integers(0, 1 << 63, size=len(todo), dtype=np.int64).astype(U) << U(1)) & ~mask | slots[todo]
        k = mix64_inv(h)
        if key_words == 2:
            second = rng.integers(1, 1 << 62, size=len(todo), dtype=np.int64).astype(U) | U(BIT63)
            with np.errstate(over="ignore"):
                k = k ^ (second * U(GOLDEN))
            good = (k & U(BIT63)) != 0
            out[todo, 1] = second
        else:
            good = k != 0
        out[todo, 0] = k
        todo = todo[~good]
    assert np.array_equal(key_hash(out, key_words) & mask, slots)
    return out if key_words == 2 else out[:, 0]


def _q_words(q):
    w = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 4).view(np.uint32).astype(U)
    return w[:, 0] | (w[:, 1] << U(32)), w[:, 2] | (w[:, 3] << U(32))


def slot_words(keys, q, key_words):
    """The four words of the slots that hold these rows: uint64 [R, 4] (reserved: 0 for 4x4)."""
    k = keys2d(keys, key_words)
    w = np.zeros((len(k), 4), U)
    w[:, 0] = k[:, 0]
    w[:, 1], w[:, 2] = _q_words(q)
    if key_words == 2:
        w[:, 3] = k[:, 1]
    return w


def build_image(cap_log2, keys, q, key_words):
    """The image a single-threaded reference leaves after inserting the rows one by one, in the order given: a row goes
    to the first empty slot of its key's sequence; a key that is already there has its values overwritten in place.
    Raises when a row finds no slot (the table is full).
    The walk along the sequence is done line by line: a full line is stepped over through a next-line-with-room link
    (with path compression), inside a line with room the first empty slot in the sequence's order is taken -- the same
    slot the slot-by-slot walk `slot_at(hash, cap_log2, 0), slot_at(hash, cap_log2, 1), ...` ends at (`build_image_walk`
    is that walk, literally; the module's test compares the two)."""
    cap = 1 << cap_log2
    lines = cap >> 2
    k2 = keys2d(keys, key_words)
    words = slot_words(k2, q, key_words)
    hashes = key_hash(k2, key_words).tolist()
    image = np.zeros((cap, 4), U)
    occupied = bytearray(cap)
    nxt = list(range(lines))                      # nxt[l]: a line at or after l (cyclically) that may have room
    room = [4] * lines
    where = {}
    key_list = [tuple(r) for r in k2.tolist()]
    for r, (key, h) in enumerate(zip(key_list, hashes)):
        assert key[0] != 0, "key 0 marks an empty slot"
        at = where.get(key)
        if at is None:
            if len(where) == cap:
                raise ValueError("the table is full")
            line, off = (h & (cap - 1)) >> 2, h & 3
            root = line
            while room[root] == 0:
                root = nxt[root] if nxt[root] != root else (root + 1) % lines
            while line != root:                   # path compression
                step = nxt[line] if nxt[line] != line else (line + 1) % lines
                nxt[line] = root
                line = step
            for j in range(4):
                at = (root << 2) | ((off + j) & 3)
                if not occupied[at]:
                    break
            occupied[at] = 1
            room[root] -= 1
            where[key] = at
        image[at] = words[r]
    return image


def build_image_walk(cap_log2, keys, q, key_words):
    """build_image by the literal slot-by-slot walk (slow: for small tables and the model's own test)."""
    cap = 1 << cap_log2
    k2 = keys2d(keys, key_words)
    words = slot_words(k2, q, key_words)
    hashes = key_hash(k2, key_words)
    image = np.zeros((cap, 4), U)
    for r in range(len(k2)):
        for p in range(cap):
            at = int(slot_at(hashes[r], cap_log2, p))
            if image[at, 0] == 0 or (image[at, 0] == k2[r, 0] and (key_words == 1 or image[at, 3] == k2[r, 1])):
                image[at] = words[r]
                break
        else:
            raise ValueError("the table is full")
    return image


def sort_rows(keys, q, key_words):
    """(keys [R, key_words], q [R, 4]) ordered by key (first word, then second)."""
    k = keys2d(keys, key_words)
    q = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 4)
    order = np.lexsort(k.T[::-1])
    return k[order], q[order]


def rows_of(image, key_words):
    """The occupied slots of an image as (keys uint64 [R, key_words], q float32 [R, 4]) sorted by key, read from the raw
    words alone."""
    occ = image[:, 0] != 0
    rows = image[occ]
    keys = rows[:, [0, 3][:key_words]]
    q = np.ascontiguousarray(rows[:, 1:3]).view(np.float32).reshape(-1, 4)
    return sort_rows(keys, q, key_words)


def positions(image, key_words):
    """(slots, position of each occupied slot on its own key's sequence)."""
    cap_log2 = int(len(image)).bit_length() - 1
    occ = np.flatnonzero(image[:, 0] != 0)
    h = key_hash(image[occ][:, [0, 3][:key_words]], key_words)
    return occ, pos_of(h, cap_log2, occ).astype(np.int64)


def check_structure(image, key_words, max_pos, summarised=False):
    """Asserts what an open-addressed table without deletion lives by, each with the first offending slot:
      - no key occurs twice (5x5: the pair of words);
      - every occupied slot lies at a position p < max_pos of its own key's sequence and every position before p on
        that sequence is occupied;
      - 5x5: both key words of an occupied slot carry bit 63 (so no occupied slot has a zero second word);
      - 4x4: `reserved` is 0 everywhere, or the line's summary word everywhere when the table is `summarised`."""
    cap = len(image)
    cap_log2 = cap.bit_length() - 1
    assert cap == 1 << cap_log2 and image.shape == (cap, 4) and image.dtype == U
    occ_mask = image[:, 0] != 0
    occ = np.flatnonzero(occ_mask)
    if key_words == 2:
        zero2 = occ[image[occ, 3] == 0]
        assert len(zero2) == 0, f"slot {zero2[0]}: occupied 5x5 slot with a zero second key word"
        nobit = occ[((image[occ, 0] & image[occ, 3]) >> U(63)) == 0]
        assert len(nobit) == 0, f"slot {nobit[0]}: a 5x5 key word without bit 63"
    else:
        want = np.repeat(line_summaries(image, 1), 4) if summarised else np.zeros(cap, U)
        bad = np.flatnonzero(image[:, 3] != want)
        assert len(bad) == 0, (f"slot {bad[0]}: reserved = {int(image[bad[0], 3]):#x}, expected {int(want[bad[0]]):#x} "
                               f"({'the line summary' if summarised else 'a 4x4 table without summaries'})")
    if len(occ) == 0:
        return
    keys = image[occ][:, [0, 3][:key_words]]
    order = np.lexsort(keys.T[::-1])
    ks = keys[order]
    dup = np.flatnonzero((ks[1:] == ks[:-1]).all(axis=1))
    assert len(dup) == 0, (f"slot {min(occ[order[dup[0]]], occ[order[dup[0] + 1]])}: its key "
                           f"{[hex(int(w)) for w in ks[dup[0]]]} occurs again in slot "
                           f"{max(occ[order[dup[0]]], occ[order[dup[0] + 1]])}")
    h = key_hash(keys, key_words)
    pos = pos_of(h, cap_log2, occ).astype(np.int64)
    deep = np.flatnonzero(pos >= min(max_pos, cap))
    assert len(deep) == 0, f"slot {occ[deep[0]]}: at position {pos[deep[0]]} of its sequence, the limit is {min(max_pos, cap)}"
    # every position before p: the p // 4 lines from the home line on are full, and so are the first p % 4 slots, in
    # the sequence's order, of the line the row lies in
    lines = cap >> 2
    full = occ_mask.reshape(lines, 4).all(axis=1)
    csum = np.concatenate([[0], np.cumsum(np.concatenate([full, full]))])
    line0 = ((h & U(cap - 1)) >> U(2)).astype(np.int64)
    ok = csum[line0 + (pos >> 2)] - csum[line0] == (pos >> 2)
    off = (h & U(3)).astype(np.int64)
    last = (occ >> 2) << 2
    for j in range(3):
        ok &= (j >= (pos & 3)) | occ_mask[last | ((off + j) & 3)]
    bad = np.flatnonzero(~ok)
    if len(bad):
        b = bad[0]
        for p in range(int(pos[b])):
            s = int(slot_at(h[b], cap_log2, p))
            assert occ_mask[s], (f"slot {occ[b]}: its row lies at position {pos[b]} of its key's sequence, but slot {s} at "
                                 f"position {p} of that sequence is empty (the row cannot be found)")
        raise AssertionError(f"slot {occ[b]}: unreachable row")


def random_rows(rng, rows, key_words):
    """Distinct random keys (5x5: both words with bit 63) and values."""
    keys = rng.integers(1, 1 << 62, size=(2 * rows + 8, key_words), dtype=np.int64).astype(U)
    if key_words == 2:
        keys |= U(BIT63)
    _, first = np.unique(keys, axis=0, return_index=True)
    keys = keys[np.sort(first)][:rows]
    assert len(keys) == rows
    return (keys if key_words == 2 else keys[:, 0]), rng.standard_normal((rows, 4)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
# The 4-call API (q_choose / q_update and their row cache), restated from include/q2048.h and the comments of
# csrc/q2048_core.hpp / q2048_core5.hpp.
#   state key   4x4: key4_of_cells ^ salt, and 1 where that is 0 (0 marks an empty slot).  5x5: word 0 ^ (salt with bit 63
#               cleared), word 1 ^ (mix64(salt) with bits 62 and 63 cleared): both words keep their bit 63.
#   salt        0, or with Q2048_FLAG_INDEPENDENT mix64(global env id + 0x2048) | 1.
#   record      one per env.  n = 4 (32 bytes): key, four float32 values, slot.  n = 5 (48 bytes): key, four values, the
#               second key word, slot, a pad that is 0.  `slot` = the row's slot index in its low 40 bits -- all ones for
#               a ROWLESS record, the visit row of a state without a row -- and the table's 24-bit tag above them.
#               A record whose key is 0 is empty, whatever else it holds.
#   td_value    Agent/main.py:41-43 in float64 with the product and the sum rounded separately, rounded to float32 once.
# ---------------------------------------------------------------------------------------------------------------
FLAG_INDEPENDENT, FLAG_TD_CAS, FLAG_NO_NEW_ROWS = 1, 4, 128
CACHE_SLOT_MASK = (1 << 40) - 1
ROWLESS = CACHE_SLOT_MASK
RECORD = {4: np.dtype([("key", "<u8"), ("q", "<f4", (4,)), ("slot", "<u8")]),
          5: np.dtype([("key", "<u8"), ("q", "<f4", (4,)), ("key_hi", "<u8"), ("slot", "<u8"), ("pad", "<u8")])}
assert RECORD[4].itemsize == 32 and RECORD[5].itemsize == 48


def lane_salt(env_ids):
    """The salt of Q2048_FLAG_INDEPENDENT for these global env ids (uint64, wrapping)."""
    with np.errstate(over="ignore"):
        return mix64(np.asarray(env_ids, dtype=U) + U(0x2048)) | U(1)


def state_key(cells, n, salt=None):
    """The table key of boards [R, n * n] (uint8 log2 tiles): uint64 [R] for n = 4, [R, 2] for n = 5.  salt: None (a
    shared table) or uint64 [R]."""
    if n == 4:
        k = key4_of_cells(cells)
        if salt is not None:
            k = k ^ np.asarray(salt, dtype=U)
        return np.where(k == 0, U(1), k)
    k = key5_of_cells(cells)
    if salt is not None:
        salt = np.asarray(salt, dtype=U)
        k = np.stack([k[:, 0] ^ (salt & U(BIT63 - 1)), k[:, 1] ^ (mix64(salt) & U((1 << 62) - 1))], axis=1)
    return k


def cache_tag(address, cap_log2):
    """The 24-bit tag (in bits 40..63) of the table at `address` with 2^cap_log2 slots."""
    mask = (1 << cap_log2) - 1
    return int(mix64(U((address ^ (mask * GOLDEN)) & _M64))) & ~CACHE_SLOT_MASK & _M64


def pack_records(n, keys, q, slots, tag):
    """Records for these rows: keys [R] / [R, 2], q float32 [R, 4], slots int (ROWLESS for a visit row), one tag."""
    k = keys2d(keys, 1 if n == 4 else 2)
    rec = np.zeros(len(k), RECORD[n])
    rec["key"] = k[:, 0]
    if n == 5:
        rec["key_hi"] = k[:, 1]
    rec["q"] = np.ascontiguousarray(q, dtype=np.float32).reshape(-1, 4)
    rec["slot"] = np.asarray(slots, dtype=U) | U(tag)
    return rec


def unpack_records(n, rec):
    """-> dict of keys [R, key_words], q bits uint32 [R, 4], slot (low 40 bits), tag, rowless, pad (n = 5, else zeros)."""
    rec = np.asarray(rec).view(RECORD[n]).reshape(-1)
    keys = rec["key"][:, None] if n == 4 else np.stack([rec["key"], rec["key_hi"]], axis=1)
    slot = rec["slot"] & U(CACHE_SLOT_MASK)
    return dict(keys=keys, qbits=np.ascontiguousarray(rec["q"]).view(np.uint32), slot=slot,
                tag=rec["slot"] & ~U(CACHE_SLOT_MASK), rowless=slot == U(ROWLESS),
                pad=rec["pad"] if n == 5 else np.zeros(len(rec), U))


def td_value(q_sa, reward, max_next, done, lr, gamma):
    """The new Q[s][a]: float32 inputs widened to float64, `gamma * max_next`, `reward + that * (0 if done else 1)`,
    `lr * (target - q)` and `q + that` each rounded on its own (Python floats: no fused multiply-add), then one
    rounding to float32."""
    q, r, m = float(np.float32(q_sa)), float(np.float32(reward)), float(np.float32(max_next))
    bootstrap = float(gamma) * m
    target = r + bootstrap * (0.0 if done else 1.0)
    step = float(lr) * (target - q)
    return np.float32(q + step)


def find_slot(image, key, key_words):
    """The slot that holds `key` (a tuple of key_words ints) in an image, or -1: by scanning the words, not by probing."""
    hit = image[:, 0] == U(key[0])
    if key_words == 2:
        hit &= image[:, 3] == U(key[1])
    at = np.flatnonzero(hit)
    assert len(at) <= 1
    return int(at[0]) if len(at) else -1
