"""The kernels of the 4-call API -- q_choose, q_update with its row cache, rowcache_rebind, env_step, env_reset and the
one-hot encoder -- each against a model of its own, on RAW BYTES.

The entry points are called through ctypes on buffers the test wrote: tables and row caches are built by
tests/table_model.py (a numpy restatement of the layout that shares no code with the product), boards and aux records
come from the oracle, and what a call leaves is read back as bytes.  The model of a decision or an update is
oracle/oracle.py (`O.draws`, `O.draw_uniform`, `O.draw_action`, `O.Env`) and `M.td_value`.  Every comparison is exact --
integers, and float32 as bit patterns -- and covers every lane; there is no tolerance anywhere in this file.  Every test
runs on the CPU twin ("cpu") and on the GPU, so both libraries are held to the same model.

Batch sizes sit either side of a wave (63, 64, 65), of the 256-lane workgroup (255, 256, 257) and, for q_update, of its
1024-lane workgroup (1023, 1024, 1025, 2049): every kernel runs with a partial last wave, q_update with a partial last
block."""
import os

import numpy as np
import pytest
import torch

import table_model as M
from table_model import U
from test_table_kernels import DEVICES, i64, lib, new_table, raw, write

BAD_ACTION, TILE_OVERFLOW, TABLE_FULL = 1, 2, 4
INDEPENDENT, TD_CAS, ENV_DQN, RESET_SHAPING, NO_NEW_ROWS = 1, 4, 8, 16, 128
ST_INSERTS, ST_DROPS, ST_CAS_RETRY, NSTAT = 4, 5, 7, 32
CANARY = 0xEE
CHOOSE_B = [1, 63, 64, 65, 255, 256, 257, 1000]
UPDATE_B = [1, 63, 64, 65, 1023, 1024, 1025, 2049]
STEP_B = [1, 63, 64, 65, 255, 256, 257]
ID_FAR = (1 << 33) + 5
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------
def dev_of(dev, a, dtype):
    """A device tensor holding the bytes of `a` (numpy, any dtype of the same width as the torch `dtype`)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev).view(dtype).reshape(a.shape)


def u8(dev, a):
    return dev_of(dev, np.asarray(a, dtype=np.uint8), torch.uint8)


def u32(dev, a):
    return dev_of(dev, np.asarray(a, dtype=np.uint32), torch.int32)


def f32(dev, a):
    return dev_of(dev, np.asarray(a, dtype=np.float32), torch.float32)


def canary(dev, count, dtype=torch.uint8):
    """`count` elements of `dtype`, every BYTE the canary."""
    return torch.full((count * torch.empty(0, dtype=dtype).element_size(),), CANARY, dtype=torch.uint8, device=dev).view(dtype)


def host_bytes(t):
    return t.cpu().contiguous().view(torch.uint8).numpy().copy()


def assert_canary_beyond(t, count, what):
    """Everything of tensor `t` beyond its first `count` elements still holds the canary."""
    tail = host_bytes(t.reshape(-1)[count:])
    assert (tail == CANARY).all(), f"{what}: written beyond element {count}"


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def words_of(n):
    return 1 if n == 4 else 2


def key_tuples(keys, n):
    return [tuple(int(w) for w in r) for r in M.keys2d(keys, words_of(n))]


def random_boards(rng, count, n):
    """`count` distinct boards of log2 tiles 0..15 (4x4) / 0..17 (5x5), none of them empty."""
    cells = rng.integers(0, 16 if n == 4 else 18, size=(2 * count + 8, n * n)).astype(np.uint8)
    cells[:, 0] |= 1
    _, first = np.unique(cells, axis=0, return_index=True)
    cells = cells[np.sort(first)][:count]
    assert len(cells) == count
    return cells


def slot_map(image, n):
    """key tuple -> slot of every occupied slot of an image, from the words alone."""
    occ = np.flatnonzero(image[:, 0] != 0)
    cols = [0, 3][:words_of(n)]
    return {tuple(int(w) for w in image[s, cols]): int(s) for s in occ}


def rows_dict(image, n):
    keys, q = M.rows_of(image, words_of(n))
    return {k: q[r].copy() for r, k in enumerate(key_tuples(keys, n))}


def assert_rows_equal_dict(image, d, n, what):
    """The occupied slots of an image are exactly the model's dict, bit for bit."""
    keys, q = M.rows_of(image, words_of(n))
    want_keys = np.array(sorted(d), dtype=U).reshape(-1, words_of(n))
    wk, wq = M.sort_rows(want_keys, np.array([d[tuple(int(w) for w in k)] for k in want_keys], dtype=np.float32).reshape(-1, 4),
                         words_of(n))
    assert len(keys) == len(wk), f"{what}: {len(keys)} rows in the bytes, the model has {len(wk)}"
    assert np.array_equal(keys, wk), f"{what}: key sets differ"
    bad = bits(q) != bits(wq)
    assert not bad.any(), f"{what}: {int(bad.any(axis=1).sum())} rows differ in their bits, first at {np.argwhere(bad)[0]}"


# ---------------------------------------------------------------------------------------------------------------
# 1. choose
# ---------------------------------------------------------------------------------------------------------------
def decision_rows():
    """Rows designed for argmax4: all equal; two equal maxima in every pair of positions; a maximum in each position;
    all negative; -0.0 beside +0.0."""
    rows = [[0.5] * 4]
    for i in range(4):
        for j in range(i + 1, 4):
            r = [0.25] * 4
            r[i] = r[j] = 1.0
            rows.append(r)
    for i in range(4):
        r = [1.0, -2.0, 0.0, 1.5]
        r[i] = 2.0
        rows.append(r)
    rows += [[-3.0, -1.0, -2.0, -4.0], [-1.0, -2.0, -3.0, -0.5], [-2.0, -2.0, -1.0, -1.0]]
    rows += [[-0.0, 0.0, -0.0, 0.0], [-1.0, -0.0, 0.0, -1.0], [0.0, -0.0, 0.0, -0.0], [-1.0, -1.0, -0.0, 0.0]]
    return np.array(rows, dtype=np.float32)


_WORLDS = {}


def choose_world(n):
    """A 2^8-slot image written by the model, with rows at position 0 of their sequence, later in the home line, in the
    next line and across the table's wrap; the boards that have a row, boards that have none, and the row of every key."""
    if n not in _WORLDS:
        cap_log2, words = 8, words_of(n)
        cap = 1 << cap_log2
        for seed in range(64):
            rng = np.random.default_rng(100 * n + seed)
            if n == 4:
                # five keys whose home is one slot (the fifth lies in the next line), five at home in the table's last
                # line (the fifth wraps to line 0), and random boards
                special = M.cells_of_key4(M.keys_with_home(rng, cap_log2, 1, [21] * 5 + [cap - 1] * 5))
                cells = np.concatenate([special, random_boards(rng, 170, n)])
            else:
                cells = random_boards(rng, 215, n)
            absent = random_boards(np.random.default_rng(7 + n), 40, n)
            keys = M.state_key(cells, n)
            if len(np.unique(M.keys2d(np.concatenate([keys, M.state_key(absent, n)]), words), axis=0)) != len(cells) + 40:
                continue
            q = decision_rows()[np.arange(len(cells)) % len(decision_rows())]
            image = M.build_image(cap_log2, keys, q, words)
            slots, pos = M.positions(image, words)
            home = M.slot_at(M.key_hash(image[slots][:, [0, 3][:words]], words), cap_log2, 0).astype(np.int64)
            wrapped = (slots >> 2) < (home >> 2)
            if (pos == 0).any() and ((pos > 0) & (pos < 4)).any() and (pos >= 4).any() and wrapped.any():
                break
        else:
            raise AssertionError("no seed gave rows of every kind")
        M.check_structure(image, words, M.ROLLOUT_PROBE)
        _WORLDS[n] = dict(cap_log2=cap_log2, image=image, present=cells, absent=absent,
                          rows=dict(zip(key_tuples(keys, n), q)))
    return _WORLDS[n]


def lane_boards(world, B, absent_every=5):
    """Boards for B lanes: rows of every decision pattern, every `absent_every`-th lane a board without a row."""
    i = np.arange(B)
    boards = world["present"][(i * 7 + 3) % len(world["present"])].copy()
    gone = i % absent_every == absent_every - 1
    boards[gone] = world["absent"][i[gone] % len(world["absent"])]
    return boards


def greedy(world, boards, n):
    """First maximum of the key's row (np.argmax: -0.0 and +0.0 compare equal); an absent key reads as zeros: action 0."""
    out = np.zeros(len(boards), np.uint8)
    for i, k in enumerate(key_tuples(M.state_key(boards, n), n)):
        out[i] = int(np.argmax(world["rows"][k])) if k in world["rows"] else 0
    return out


def call_choose(L, dev, table, cap_log2, boards, n, eps, *, draws=None, seed=0, env_id0=0, ctr=0, flags=0, cache=None):
    """One of q2048_q_choose / _draws / _cached on B lanes -> (actions [B], status).  Asserts what every call owes:
    Q2048_OK, the actions beyond B untouched, the table's bytes (and the cache's) as they were."""
    B = len(boards)
    tb = u8(dev, boards)
    actions, st = canary(dev, B + 64), torch.zeros(1, dtype=torch.int32, device=dev)
    before = raw(table)
    cache_before = None if cache is None else host_bytes(cache)
    if draws is not None:
        de, da = u32(dev, draws[0]), u32(dev, draws[1])
        rc = L.q2048_q_choose_draws(table.data_ptr(), cap_log2, tb.data_ptr(), de.data_ptr(), da.data_ptr(), B, n, eps,
                                    env_id0, flags, actions.data_ptr(), st.data_ptr(), None)
    elif cache is not None:
        rc = L.q2048_q_choose_cached(table.data_ptr(), cap_log2, tb.data_ptr(), B, n, eps, seed, env_id0, ctr, flags,
                                     cache.data_ptr(), actions.data_ptr(), st.data_ptr(), None)
    else:
        rc = L.q2048_q_choose(table.data_ptr(), cap_log2, tb.data_ptr(), B, n, eps, seed, env_id0, ctr, flags,
                              actions.data_ptr(), st.data_ptr(), None)
    assert rc == 0
    got = host_bytes(actions)
    assert (got[B:] == CANARY).all(), "actions written beyond B"
    assert np.array_equal(raw(table), before), "choose wrote the table"
    if cache is not None:
        assert np.array_equal(host_bytes(cache), cache_before), "choose wrote the row cache"
    return got[:B], int(st.item())


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_choose_with_injected_draws(pkg, O, dev, n):
    """q2048_q_choose_draws: eps in {0, 1, 0.25, 2^-33}, draw_eps at 0, T - 1, T and 2^32 - 1 (T = ceil(eps 2^32), where
    in range), draw_act at the four quarter boundaries; greedy lanes read rows built for the decision."""
    L, world = lib(pkg, dev), choose_world(n)
    table = new_table(dev, world["cap_log2"], world["image"])
    quarters = [0, (1 << 30) - 1, 1 << 30, (1 << 31) - 1, 1 << 31, 3 * (1 << 30) - 1, 3 * (1 << 30), (1 << 32) - 1]
    assert [O.draw_action(x) for x in quarters] == [0, 0, 1, 1, 2, 2, 3, 3]
    for B in CHOOSE_B:
        boards = lane_boards(world, B)
        best = greedy(world, boards, n)
        if B >= 63:
            assert set(best.tolist()) == {0, 1, 2, 3}
        for eps in (0.0, 1.0, 0.25, 2.0 ** -33):
            T = int(np.ceil(eps * 2.0 ** 32))
            edge = sorted({x for x in (0, T - 1, T, (1 << 32) - 1) if 0 <= x < (1 << 32)})
            i = np.arange(B)
            de = np.array(edge, dtype=np.uint32)[(i + (B == 1)) % len(edge)]
            da = np.array(quarters, dtype=np.uint32)[(i // len(edge) + 3) % 8]
            explore = np.array([O.draw_uniform(int(x)) < eps for x in de])
            assert np.array_equal(explore, de.astype(np.int64) < T)          # the integer threshold is the same test
            want = np.where(explore, [O.draw_action(int(x)) for x in da], best).astype(np.uint8)
            got, status = call_choose(L, dev, table, world["cap_log2"], boards, n, eps, draws=(de, da))
            assert status == 0
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, f"B={B} eps={eps}: {len(bad)} lanes differ, first lane {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_choose_with_its_own_draws(pkg, O, dev, n):
    """q2048_q_choose at a counter above 0, from env id 0 and from (1 << 33) + 5: lane i takes the draws of
    O.draws(seed, env_id0 + i, ctr)."""
    L, world = lib(pkg, dev), choose_world(n)
    table = new_table(dev, world["cap_log2"], world["image"])
    seed, ctr, eps = 11, 7, 0.25
    for env_id0 in (0, ID_FAR):
        for B in CHOOSE_B:
            boards = lane_boards(world, B)
            best = greedy(world, boards, n)
            x = np.array([O.draws(seed, env_id0 + i, ctr) for i in range(B)], dtype=np.uint32)
            explore = np.array([O.draw_uniform(int(v)) < eps for v in x[:, 0]])
            if B >= 63:
                assert explore.any() and not explore.all()
            want = np.where(explore, [O.draw_action(int(v)) for v in x[:, 1]], best).astype(np.uint8)
            got, status = call_choose(L, dev, table, world["cap_log2"], boards, n, eps, seed=seed, env_id0=env_id0, ctr=ctr)
            assert status == 0
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, f"B={B} id0={env_id0}: {len(bad)} lanes differ, first lane {bad[0]}"


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_choose_reads_private_rows(pkg, dev, n):
    """Q2048_FLAG_INDEPENDENT: ONE board in every lane, a table that holds salted rows for two lanes in three (and the
    unsalted row, which no lane may read).  A lane with a row follows it, a lane without takes action 0."""
    L, cap_log2, words = lib(pkg, dev), 12, words_of(n)
    board = random_boards(np.random.default_rng(20 + n), 1, n)
    for env_id0 in (0, ID_FAR):
        lanes = np.arange(max(CHOOSE_B))
        salt = M.lane_salt(np.asarray(lanes, dtype=U) + U(env_id0))
        keys = M.keys2d(M.state_key(np.repeat(board, len(lanes), axis=0), n, salt), words)
        assert len(np.unique(keys, axis=0)) == len(lanes)
        has = lanes % 3 != 1
        q = np.full((len(lanes), 4), -1.0, np.float32)
        q[lanes, 1 + lanes % 3] = 0.5                                  # the maximum never at action 0
        plain = M.keys2d(M.state_key(board, n), words)
        image = M.build_image(cap_log2, np.concatenate([plain, keys[has]]),
                              np.concatenate([np.array([[9.0, 0.0, 0.0, 0.0]], np.float32), q[has]]), words)
        table = new_table(dev, cap_log2, image)
        for B in CHOOSE_B:
            want = np.where(has[:B], 1 + lanes[:B] % 3, 0).astype(np.uint8)
            got, status = call_choose(L, dev, table, cap_log2, np.repeat(board, B, axis=0), n, 0.0, env_id0=env_id0,
                                      flags=INDEPENDENT)
            assert status == 0 and np.array_equal(got, want), f"B={B} id0={env_id0}"
        got, _ = call_choose(L, dev, table, cap_log2, np.repeat(board, 65, axis=0), n, 0.0, env_id0=env_id0)
        assert (got == 0).all(), "without the flag every lane reads the unsalted row"


@pytest.mark.parametrize("dev", DEVICES)
def test_choose_reads_a_row_beyond_its_probe_limit_as_absent(pkg, dev):
    """4x4, 2^12 slots: a key placed at position 1024 of its sequence, one beyond the learning paths' limit.
    q2048_q_lookup (2^14 positions) finds it; choose reads the state as absent: action 0, though the row's maximum is
    action 2.  The key one position before it is still read."""
    L, cap_log2, n = lib(pkg, dev), 12, 4
    rng = np.random.default_rng(12)
    home = 4 * 700 + 2
    run = [int(M.slot_at(U(home), cap_log2, p)) for p in range(M.ROLLOUT_PROBE - 1)]
    filler = M.keys_with_home(rng, cap_log2, 1, run)                  # each at its own home: the sequence's first 1023 slots
    last_in, deep = M.keys_with_home(rng, cap_log2, 1, [home, home])
    keys = np.concatenate([filler, [last_in, deep]])
    q = np.zeros((len(keys), 4), np.float32)
    q[-2:] = [[0.0, 0.0, 5.0, 0.0], [0.0, 0.0, 5.0, 0.0]]
    image = M.build_image(cap_log2, keys, q, 1)
    slots, pos = M.positions(image, 1)
    where = dict(zip(image[slots, 0].tolist(), pos.tolist()))
    assert where[int(last_in)] == M.ROLLOUT_PROBE - 1 and where[int(deep)] == M.ROLLOUT_PROBE
    table = new_table(dev, cap_log2, image)
    boards = M.cells_of_key4(np.array([last_in, deep], dtype=U))
    tb = u8(dev, boards)
    out, found = f32(dev, np.zeros((2, 4))), u8(dev, [9, 9])
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    assert L.q2048_q_lookup(table.data_ptr(), cap_log2, tb.data_ptr(), 2, n, 0, 0, out.data_ptr(), found.data_ptr(),
                            st.data_ptr(), None) == 0
    assert found.cpu().tolist() == [1, 1] and np.array_equal(bits(out.cpu().numpy()), bits(q[-2:]))
    got, status = call_choose(L, dev, table, cap_log2, boards, n, 0.0)
    assert status == 0 and got.tolist() == [2, 0]


def cache_of(dev, rec, extra=0):
    """A device row cache holding these records, followed by `extra` records of canary bytes."""
    body = np.ascontiguousarray(rec).view(np.uint8).reshape(-1)
    tail = np.full(extra * rec.dtype.itemsize, CANARY, np.uint8)
    return torch.from_numpy(np.concatenate([body, tail])).to(dev)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_choose_with_hand_built_records(pkg, dev, n):
    """q2048_q_choose_cached on records the test wrote, one kind per lane: empty; a hit (key and tag) whose values are
    not the table's row -- the record decides; the right key under another table's tag; a record of another key (5x5:
    only its second word differs); a rowless record of a state without a row, used only with Q2048_FLAG_NO_NEW_ROWS;
    a hit for a state the table has no row for."""
    L, world = lib(pkg, dev), choose_world(n)
    cap_log2, words = world["cap_log2"], words_of(n)
    table = new_table(dev, cap_log2, world["image"])
    tag = M.cache_tag(table.data_ptr(), cap_log2)
    other_tag = M.cache_tag(table.data_ptr() + (1 << 20), cap_log2)
    assert tag != other_tag and tag != M.cache_tag(table.data_ptr(), cap_log2 + 1)
    slots = slot_map(world["image"], n)
    for B in CHOOSE_B:
        boards = lane_boards(world, B, absent_every=10 ** 9)
        kind = np.arange(B) % 6
        boards[kind >= 4] = world["absent"][np.arange(B)[kind >= 4] % len(world["absent"])]
        keys = M.keys2d(M.state_key(boards, n), words)
        table_best = greedy(world, boards, n)
        rec_q = np.zeros((B, 4), np.float32)
        rec_q[np.arange(B), (table_best + 1 + np.arange(B) % 3) % 4] = 3.0   # a maximum where the table's row has none
        rec_best = np.argmax(rec_q, axis=1)
        assert (rec_best != table_best).all()
        rec = M.pack_records(n, keys, rec_q, [slots.get(k, 3) for k in key_tuples(keys, n)], tag)
        rec[kind == 0] = np.zeros(1, M.RECORD[n])
        rec["slot"][kind == 2] = (rec["slot"][kind == 2] & U(M.CACHE_SLOT_MASK)) | U(other_tag)
        if n == 5:
            rec["key_hi"][kind == 3] ^= U(1 << 7)
        else:
            rec["key"][kind == 3] ^= U(1 << 7)
        rec["slot"][kind == 4] = U(M.ROWLESS | tag)
        cache = cache_of(dev, rec)
        for flags in (0, NO_NEW_ROWS):
            want = np.where((kind == 1) | (kind == 5) | ((kind == 4) & (flags != 0)), rec_best, table_best).astype(np.uint8)
            got, status = call_choose(L, dev, table, cap_log2, boards, n, 0.0, seed=3, ctr=2, flags=flags, cache=cache)
            bad = np.flatnonzero(got != want)
            assert status == 0 and len(bad) == 0, f"B={B} flags={flags}: lane {bad[:1]} of kind {kind[bad[:1]]}"


# ---------------------------------------------------------------------------------------------------------------
# 2. update
# ---------------------------------------------------------------------------------------------------------------
REWARDS = np.array([-1.5, 0.375, 2048.0, -0.1, 7.25], dtype=np.float32)
DONES = np.array([0, 1, 255, 0, 0, 1, 0], dtype=np.uint8)


def cap_for(rows):
    return max(6, int(2 * rows - 1).bit_length())


def transitions(n, B, independent, seed):
    """B transitions no two of which touch one key, and the rows the table holds before the call.
    Shared table: distinct boards; at 4x4 the keys come in pairs that share a home slot, so two new rows compete for it.
    Independent: ONE pair of boards in every lane, the keys differ by the lane's salt.
    Per lane: s present or absent; s' present with its maximum in each position or all negative, absent, or s itself
    (one lane in five); rewards negative, fractional and 2048; done bytes 0, 1 and 255; one lane in eleven has action 4
    or 255."""
    rng = np.random.default_rng(seed)
    words, lane = words_of(n), np.arange(B)
    cap_log2 = cap_for(2 * B)
    if independent:
        pair = random_boards(rng, 2, n)
        s, s2 = np.repeat(pair[:1], B, axis=0), np.repeat(pair[1:], B, axis=0)
    elif n == 4:
        homes = rng.integers(0, 1 << cap_log2, size=B)
        s = M.cells_of_key4(M.keys_with_home(rng, cap_log2, 1, homes))
        s2 = M.cells_of_key4(M.keys_with_home(rng, cap_log2, 1, np.concatenate([homes[1:], homes[:1]])))
    else:
        both = random_boards(rng, 2 * B, n)
        s, s2 = both[:B], both[B:]
    same = lane % 5 == 4
    s2[same] = s[same]
    actions = (lane % 4).astype(np.uint8)
    actions[lane % 11 == 7] = np.where(lane[lane % 11 == 7] % 2 == 0, 4, 255)
    reward, done = REWARDS[lane % len(REWARDS)], DONES[lane % len(DONES)]
    # the rows written beforehand: s of every second lane; s' of two lanes in three
    q_s = rng.standard_normal((B, 4)).astype(np.float32)
    q_n = rng.standard_normal((B, 4)).astype(np.float32)
    q_n[lane, lane % 4] = 4.0                                         # the maximum in each position ...
    neg = (lane // 3) % 2 == 1
    q_n[neg] = -np.abs(q_n[neg]) - 0.5                                # ... or an all-negative row
    s_there = lane % 2 == 0
    n_there = (lane % 3 != 0) & ~same
    return dict(cap_log2=cap_log2, s=s, s2=s2, same=same, actions=actions, reward=reward, done=done, q_s=q_s, q_n=q_n,
                s_there=s_there, n_there=n_there, independent=independent)


def lane_keys(t, n, env_id0):
    salt = M.lane_salt(np.arange(len(t["s"]), dtype=U) + U(env_id0)) if t["independent"] else None
    ks, kn = key_tuples(M.state_key(t["s"], n, salt), n), key_tuples(M.state_key(t["s2"], n, salt), n)
    # the model's precondition: no two lanes touch one key
    touched = [k for a, b in zip(ks, kn) for k in {a, b}]
    assert len(set(touched)) == len(touched), "two lanes touch one key"
    assert [a == b for a, b in zip(ks, kn)] == t["same"].tolist()
    return ks, kn


def written_image(t, n, ks, kn):
    words = words_of(n)
    keys = [ks[i] for i in np.flatnonzero(t["s_there"])] + [kn[i] for i in np.flatnonzero(t["n_there"])]
    q = np.concatenate([t["q_s"][t["s_there"]], t["q_n"][t["n_there"]]]).reshape(-1, 4)
    return M.build_image(t["cap_log2"], np.array(keys, dtype=U).reshape(-1, words), q, words)


def model_update(d, ks, kn, actions, reward, done, lr, gamma, flags, records=None, room=True):
    """Agent/main.py:40-43 for every lane, ONE pass over ONE dict (the keys of two lanes are disjoint, so the order of
    the lanes does not matter).  `records`: per lane None, or (key, float32 [4], slot or None for rowless) -- a record
    that matched: the row is the record's, not the table's.  `room` False: the table is full, no row can be created.
    -> (status, inserts, drops, per lane None (lane untouched) or (key of s', its row float32 [4], 'has a row'))."""
    create = not flags & NO_NEW_ROWS
    status = inserts = drops = 0
    left = []

    def read(k):
        nonlocal inserts
        if k in d:
            return d[k].copy(), True
        if create and room:
            d[k] = np.zeros(4, np.float32)
            inserts += 1
            return d[k].copy(), True
        return np.zeros(4, np.float32), False

    for i in range(len(ks)):
        a = int(actions[i])
        if a > 3:
            status |= BAD_ACTION
            left.append(None)
            continue
        hit = records[i] if records is not None else None
        if hit is not None and hit[0] == ks[i] and (hit[2] is not None or not create):
            rs, s_row = hit[1].copy(), hit[2] is not None
        else:
            rs, s_row = read(ks[i])
        if kn[i] == ks[i]:
            rn, n_row = rs.copy(), s_row
        else:
            rn, n_row = read(kn[i])
        nq = M.td_value(rs[a], reward[i], np.max(rn), done[i] != 0, lr, gamma)
        if s_row:
            d[ks[i]][a] = nq
            if kn[i] == ks[i]:
                rn[a] = nq
        else:
            drops += 1
            if create:
                status |= TABLE_FULL
            elif kn[i] == ks[i]:
                rn[a] = nq                                            # the visit row learns
        left.append((kn[i], rn, n_row))
    return status, inserts, drops, left


def call_update(L, dev, table, cap_log2, t, n, lr, gamma, env_id0, flags, cache=None, stats0=None):
    B = len(t["s"])
    ts, tn = u8(dev, t["s"]), u8(dev, t["s2"])
    ta, tr, td = u8(dev, t["actions"]), f32(dev, t["reward"]), u8(dev, t["done"])
    stats0 = np.arange(100, 100 + NSTAT, dtype=np.int64) if stats0 is None else stats0
    stats, st = torch.from_numpy(stats0.copy()).to(dev), torch.zeros(1, dtype=torch.int32, device=dev)
    args = (table.data_ptr(), cap_log2, ts.data_ptr(), ta.data_ptr(), tr.data_ptr(), tn.data_ptr(), td.data_ptr(), B, n, lr,
            gamma, env_id0, flags)
    if cache is None:
        rc = L.q2048_q_update(*args, stats.data_ptr(), st.data_ptr(), None)
    else:
        rc = L.q2048_q_update_cached(*args, cache.data_ptr(), stats.data_ptr(), st.data_ptr(), None)
    assert rc == 0
    for name, sent, now in (("boards_s", t["s"], ts), ("boards_s2", t["s2"], tn)):
        assert np.array_equal(now.cpu().numpy(), sent), f"{name} was written"
    return stats.cpu().numpy() - stats0, int(st.item())


def assert_stats(delta, inserts, drops, what):
    want = np.zeros(NSTAT, np.int64)
    want[ST_INSERTS], want[ST_DROPS] = inserts, drops
    assert np.array_equal(delta, want), f"{what}: statistics moved by {delta.tolist()}, the model says inserts={inserts} drops={drops}"


def assert_records(n, cache, left, before, image, tag, frozen, what):
    """The cache's bytes lane by lane: an untouched lane's record as it was; else the key of s' (5x5: both words, pad
    0), the four values of the model's row, the slot where that key lies in the bytes read back (all ones for a visit
    row) and the table's tag.  A state without a row and without a visit row leaves an empty record: key 0."""
    B = len(left)
    now = host_bytes(cache).reshape(-1, M.RECORD[n].itemsize)
    assert (now[B:] == CANARY).all(), f"{what}: records beyond B were written"
    got, slots = M.unpack_records(n, now[:B].reshape(-1)), slot_map(image, n)
    for i, rec in enumerate(left):
        if rec is None:
            assert np.array_equal(now[i], before[i]), f"{what}: lane {i} has a bad action, its record changed"
            continue
        key, row, has_row = rec
        if not has_row and not frozen:
            assert int(got["keys"][i, 0]) == 0, f"{what}: lane {i}: no row, no visit row, yet a record with a key"
            continue
        assert tuple(int(w) for w in got["keys"][i]) == key, f"{what}: lane {i}: the record's key is not the key of s'"
        assert int(got["pad"][i]) == 0
        assert np.array_equal(got["qbits"][i], bits(row)), f"{what}: lane {i}: values {got['qbits'][i]} != {bits(row)}"
        assert int(got["tag"][i]) == tag, f"{what}: lane {i}: tag"
        if has_row:
            assert int(got["slot"][i]) == slots[key], f"{what}: lane {i}: slot {int(got['slot'][i])}, the key lies in {slots[key]}"
        else:
            assert bool(got["rowless"][i]), f"{what}: lane {i}: a visit row must carry the rowless marker"


def fresh_cache(dev, n, B):
    """B empty records and 8 records of canary bytes behind them."""
    return cache_of(dev, np.zeros(B, M.RECORD[n]), extra=8)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("independent", [False, True])
def test_update_on_a_written_table(pkg, dev, n, independent):
    """q2048_q_update and q2048_q_update_cached on a table the model wrote, for every B and for the flags 0,
    Q2048_FLAG_TD_CAS and Q2048_FLAG_NO_NEW_ROWS: the rows read back from the bytes are the model's dict, the table's
    structure holds within the learning paths' probe limit, inserts and drops are the model's counts and every other
    statistic stays, the status is exactly the model's, and with a cache every record is what the header says."""
    L, words, lr = lib(pkg, dev), words_of(n), 0.1
    for B in UPDATE_B:
        env_id0 = ID_FAR if independent else 0
        t = transitions(n, B, independent, seed=1000 * n + B)
        ks, kn = lane_keys(t, n, env_id0)
        image = written_image(t, n, ks, kn)
        cap_log2 = t["cap_log2"]
        M.check_structure(image, words, M.ROLLOUT_PROBE)
        base = INDEPENDENT if independent else 0
        for flags, gamma, cached in ((0, 0.9, False), (0, 0.95, True), (TD_CAS, 0.95, False), (NO_NEW_ROWS, 0.9, True),
                                     (NO_NEW_ROWS, 0.95, False)):
            what = f"B={B} flags={flags} cached={cached}"
            table = new_table(dev, cap_log2, image)
            cache = fresh_cache(dev, n, B) if cached else None
            before = host_bytes(cache).reshape(-1, M.RECORD[n].itemsize) if cached else None
            d = rows_dict(image, n)
            status, inserts, drops, left = model_update(d, ks, kn, t["actions"], t["reward"], t["done"], lr, gamma, flags)
            delta, got_status = call_update(L, dev, table, cap_log2, t, n, lr, gamma, env_id0, base | flags, cache)
            after = raw(table)
            assert got_status == status, f"{what}: status {got_status}, the model says {status}"
            assert not status & TABLE_FULL
            assert_stats(delta, inserts, drops, what)
            assert_rows_equal_dict(after, d, n, what)
            M.check_structure(after, words, M.ROLLOUT_PROBE)
            if flags & NO_NEW_ROWS:
                assert inserts == 0 and np.array_equal(after[:, [0, 3]], image[:, [0, 3]]), f"{what}: the key set changed"
                assert drops == sum(1 for i in range(B) if t["actions"][i] <= 3 and not t["s_there"][i])
            else:
                assert drops == 0 and np.array_equal(after[image[:, 0] != 0][:, [0, 3]], image[image[:, 0] != 0][:, [0, 3]])
            if cached:
                assert_records(n, cache, left, before, after, M.cache_tag(table.data_ptr(), cap_log2),
                               bool(flags & NO_NEW_ROWS), what)
    assert pkg._native.claim_timeouts(L) == 0


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_update_of_a_full_table(pkg, dev, n):
    """A 2^4-slot table without a free slot, without Q2048_FLAG_NO_NEW_ROWS: a lane whose s has a row updates it, every
    other lane's update is dropped and counted, Q2048_STATUS_TABLE_FULL is raised, no key changes and every row the
    call did not update keeps its bits."""
    L, words, cap_log2, lr, gamma = lib(pkg, dev), words_of(n), 4, 0.1, 0.9
    for B in (2, 12, 65):
        t = transitions(n, B, False, seed=77 + n)
        ks, kn = lane_keys(t, n, 0)
        rng = np.random.default_rng(5)
        mine = [ks[i] for i in range(min(B, 6)) if t["s_there"][i]] + [kn[i] for i in range(min(B, 6)) if t["n_there"][i]]
        more = key_tuples(M.state_key(random_boards(rng, 16, n)[::-1], n), n)
        keys = (mine + [k for k in more if k not in set(ks) | set(kn)])[:16]
        image = M.build_image(cap_log2, np.array(keys, dtype=U).reshape(-1, words), rng.standard_normal((16, 4)).astype(np.float32),
                              words)
        assert (image[:, 0] != 0).all()
        for cached in (False, True):
            table, d = new_table(dev, cap_log2, image), rows_dict(image, n)
            cache = fresh_cache(dev, n, B) if cached else None
            before = host_bytes(cache).reshape(-1, M.RECORD[n].itemsize) if cached else None
            status, inserts, drops, left = model_update(d, ks, kn, t["actions"], t["reward"], t["done"], lr, gamma, 0, room=False)
            delta, got_status = call_update(L, dev, table, cap_log2, t, n, lr, gamma, 0, 0, cache)
            after = raw(table)
            assert got_status == status and status & TABLE_FULL and inserts == 0 and drops > 0
            assert_stats(delta, 0, drops, f"full table B={B}")
            assert np.array_equal(after[:, [0, 3]], image[:, [0, 3]]), "a key of a full table changed"
            assert_rows_equal_dict(after, d, n, f"full table B={B}")
            if cached:
                assert_records(n, cache, left, before, after, M.cache_tag(table.data_ptr(), cap_log2), False, f"full table B={B}")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("flags", [0, NO_NEW_ROWS])
def test_cached_update_chain(pkg, dev, n, flags):
    """Two cached updates in a row, the second from the first one's s', then a cached choose on what it left.  Between
    the two the test overwrites the rows of those states in the table's bytes: a cached row does not see later writes
    (include/q2048.h), so the second update computes from the RECORD's values and writes into the record's slot; a lane
    whose record the test zeroed probes and sees the new values.  With Q2048_FLAG_NO_NEW_ROWS the records of states
    without a row are visit rows and carry what the env's own invalid moves taught them."""
    L, words, lr, gamma = lib(pkg, dev), words_of(n), 0.1, 0.9
    frozen = bool(flags & NO_NEW_ROWS)
    for B in (1, 65, 1025):
        t1 = transitions(n, B, False, seed=300 + 10 * n + B)
        t2 = transitions(n, B, False, seed=900 + 10 * n + B)
        t2["s"] = t1["s2"].copy()
        t2["s2"][t2["same"]] = t2["s"][t2["same"]]
        ks1, kn1 = lane_keys(t1, n, 0)
        ks2, kn2 = lane_keys(t2, n, 0)
        assert ks2 == kn1 and not (set(kn2) - set(ks2)) & (set(ks1) | set(kn1))
        cap_log2 = cap_for(3 * B)
        t1["cap_log2"] = cap_log2
        image = written_image(t1, n, ks1, kn1)
        if frozen:                                                     # a closed key set that holds some of the s'' as well
            extra = [kn2[i] for i in range(B) if i % 3 == 1 and kn2[i] != ks2[i]]
            rows = M.rows_of(image, words)
            keys = np.concatenate([rows[0], np.array(extra, dtype=U).reshape(-1, words)])
            image = M.build_image(cap_log2, keys, np.concatenate([rows[1], np.full((len(extra), 4), 0.75, np.float32)]), words)
        table, cache = new_table(dev, cap_log2, image), fresh_cache(dev, n, B)
        tag = M.cache_tag(table.data_ptr(), cap_log2)
        d = rows_dict(image, n)
        status, inserts, drops, left = model_update(d, ks1, kn1, t1["actions"], t1["reward"], t1["done"], lr, gamma, flags)
        before = host_bytes(cache).reshape(-1, M.RECORD[n].itemsize)
        delta, got_status = call_update(L, dev, table, cap_log2, t1, n, lr, gamma, 0, flags, cache)
        mid = raw(table)
        assert got_status == status
        assert_stats(delta, inserts, drops, f"first B={B}")
        assert_rows_equal_dict(mid, d, n, f"first B={B}")
        assert_records(n, cache, left, before, mid, tag, frozen, f"first B={B}")
        # other values into the rows of every s' -- in the bytes and in the model's dict
        slots = slot_map(mid, n)
        rng = np.random.default_rng(B)
        for k in set(kn1) & set(slots):
            d[k] = rng.standard_normal(4).astype(np.float32)
            mid[slots[k]] = M.slot_words(np.array(k, dtype=U).reshape(1, -1), d[k], words)[0]
        write(table, mid)
        # every fourth lane loses its record
        rec_bytes = host_bytes(cache).reshape(-1, M.RECORD[n].itemsize)
        zeroed = np.arange(B) % 4 == 0
        rec_bytes[:B][zeroed] = 0
        cache.copy_(torch.from_numpy(rec_bytes.reshape(-1)))
        records = [None if zeroed[i] or rec is None or (not rec[2] and not frozen) else
                   (rec[0], rec[1], slots[rec[0]] if rec[2] else None) for i, rec in enumerate(left)]
        assert any(r is not None for r in records) or B == 1
        status, inserts, drops, left2 = model_update(d, ks2, kn2, t2["actions"], t2["reward"], t2["done"], lr, gamma, flags,
                                                     records=records)
        before = host_bytes(cache).reshape(-1, M.RECORD[n].itemsize)
        delta, got_status = call_update(L, dev, table, cap_log2, t2, n, lr, gamma, 0, flags, cache)
        after = raw(table)
        assert got_status == status
        assert_stats(delta, inserts, drops, f"second B={B}")
        assert_rows_equal_dict(after, d, n, f"second B={B}")           # (the writes landed in the records' slots)
        M.check_structure(after, words, M.ROLLOUT_PROBE)
        assert_records(n, cache, left2, before, after, tag, frozen, f"second B={B}")
        # ... and the choose that follows reads those records: the row of s'' as the update left it
        want = np.zeros(B, np.uint8)
        for i in range(B):
            rec = left2[i]
            if rec is not None and (rec[2] or frozen):
                want[i] = int(np.argmax(rec[1]))
            elif rec is not None:
                want[i] = 0
            else:                                                     # a bad action: the record is still the first call's
                old = records[i]
                row = old[1] if old is not None and old[0] == kn2[i] else d.get(kn2[i], np.zeros(4, np.float32))
                want[i] = int(np.argmax(row))
        got, status = call_choose(L, dev, table, cap_log2, t2["s2"], n, 0.0, flags=flags, cache=cache[:B * M.RECORD[n].itemsize])
        bad = np.flatnonzero(got != want)
        assert status == 0 and len(bad) == 0, f"choose after the chain, B={B}: lane {bad[:1]}"


# ---------------------------------------------------------------------------------------------------------------
# 3. step and reset
# ---------------------------------------------------------------------------------------------------------------
AUX = np.dtype([("score", "<i4"), ("ep_return", "<f4"), ("prev_max", "u1"), ("cons_action", "u1"), ("cons_count", "<u2"),
                ("episode", "<u4")])
_ENVS = {}


def midgame(O, n, B, seed, env_id0):
    """Oracle envs after 14 steps of random play (mid-game boards, scores, streaks, a few finished episodes); at 4x4
    every eighth lane's board is one of the dead boards of tests/golden/g3_game_over.npz."""
    key = (n, B, seed, env_id0)
    if key not in _ENVS:
        envs = O.envs_init(B, n, seed, env_id0)
        O.rollout(envs, None, 14, seed, env_id0, 0)
        if n == 4:
            g = np.load(os.path.join(GOLDEN_DIR, "g3_game_over.npz"))
            dead = g["boards"][g["over"].astype(bool)].reshape(-1, 16).astype(np.uint8)
            assert len(dead)
            for i in range(5, B, 8):
                envs["board"][i, :16] = dead[i % len(dead)]
        _ENVS[key] = envs
    return _ENVS[key].copy()


def aux_of(envs):
    a = np.zeros(len(envs), AUX)
    a["score"], a["ep_return"] = envs["score"], envs["episode_return"].astype(np.float32)
    a["prev_max"], a["cons_action"] = envs["previous_max_log2"], envs["consecutive_action"] & 0xFF
    a["cons_count"], a["episode"] = np.minimum(envs["consecutive_count"], 60000), envs["episode"]
    return a


def step_actions(B):
    a = ((np.arange(B) * 5 + 1) % 4).astype(np.uint8)
    bad = np.arange(B) % 13 == 6
    a[bad] = np.where(np.arange(B)[bad] % 2 == 0, 4, 255)
    return a


def model_step(O, envs, aux, actions, n, x, y, dqn):
    """One O.Env per lane.  x [B, 2]: the chosen move's spawn draws; y [B, 2]: those of the spawn inside the DQN env's
    is_game_over.  ep_return is a float32 accumulator of float32 rewards.  A lane with a bad action keeps board and aux
    and reports reward 0, done 0, max 0."""
    B, cells = len(envs), n * n
    boards, out_aux = envs["board"][:, :cells].copy(), aux.copy()
    reward, done, mx = np.zeros(B, np.float32), np.zeros(B, np.uint8), np.zeros(B, np.uint8)
    status = 0
    for i in range(B):
        if actions[i] > 3:
            status |= BAD_ACTION
            continue
        e = O.Env(n)
        e.rec[0] = envs[i]
        if dqn:
            b, r, d, m, _ = e.step_dqn(int(actions[i]), int(x[i, 0]), int(x[i, 1]), int(y[i, 0]), int(y[i, 1]))
        else:
            b, r, d, m, _ = e.step(int(actions[i]), int(x[i, 0]), int(x[i, 1]))
        boards[i], reward[i], done[i], mx[i] = b, np.float32(r), d, m
        after = aux_of(e.rec)[0]
        after["ep_return"] = np.float32(aux["ep_return"][i]) + np.float32(r)
        out_aux[i] = after
    tile = np.where(mx > 0, 1 << mx.astype(np.int64), 0).astype(np.int32)
    return boards, out_aux, reward, done, mx, tile, status


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_env_step_entry_points(pkg, O, dev, n):
    """q2048_env_step, _ex (plain and Q2048_FLAG_ENV_DQN, with its own draws and with draws4), _to (two buffers,
    max_tile) and _draws on boards and aux records the test wrote: boards, aux bytes, reward bits, done, max_log2 and
    max_tile per lane against one O.Env per lane; canaries behind lane B of every output."""
    L, cells, seed, ctr = lib(pkg, dev), n * n, 21, 9
    for B in STEP_B:
        env_id0 = ID_FAR if B % 2 else 0
        envs = midgame(O, n, B, seed, env_id0)
        aux, actions = aux_of(envs), step_actions(B)
        own = np.array([O.draws(seed, env_id0 + i, ctr) for i in range(B)], dtype=np.uint32)
        over = np.array([O.draws(seed, env_id0 + i, ctr, O.STREAM_OVER) for i in range(B)], dtype=np.uint32)
        rng = np.random.default_rng(B)
        given = rng.integers(0, 1 << 32, size=(B, 4), dtype=np.uint64).astype(np.uint32)
        for entry, dqn in (("step", False), ("ex", False), ("ex", True), ("ex4", False), ("ex4", True), ("to", False),
                           ("to", True), ("draws", False)):
            what = f"{entry} dqn={dqn} B={B}"
            injected = entry in ("ex4", "draws")
            x, y = (given[:, :2], given[:, 2:]) if injected else (own[:, 2:], over[:, :2])
            wb, wa, wr, wd, wm, wt, wstatus = model_step(O, envs, aux, actions, n, x, y, dqn)
            flags = ENV_DQN if dqn else 0
            tb = torch.cat([u8(dev, envs["board"][:, :cells]).reshape(-1), canary(dev, 64)])
            ta = torch.cat([dev_of(dev, aux.view(np.uint8).reshape(B, 16), torch.uint8).reshape(-1), canary(dev, 64)])
            tact = u8(dev, actions)
            r, d, m = canary(dev, B + 16, torch.float32), canary(dev, B + 16), canary(dev, B + 16)
            tile, st = canary(dev, B + 16, torch.int32), torch.zeros(1, dtype=torch.int32, device=dev)
            out = tb
            if entry == "step":
                rc = L.q2048_env_step(tb.data_ptr(), ta.data_ptr(), tact.data_ptr(), B, n, seed, env_id0, ctr, r.data_ptr(),
                                      d.data_ptr(), m.data_ptr(), st.data_ptr(), None)
            elif entry in ("ex", "ex4"):
                d4 = u32(dev, given) if injected else None
                rc = L.q2048_env_step_ex(tb.data_ptr(), ta.data_ptr(), tact.data_ptr(), B, n, seed, env_id0, ctr, flags,
                                         None if d4 is None else d4.data_ptr(), r.data_ptr(), d.data_ptr(), m.data_ptr(),
                                         st.data_ptr(), None)
            elif entry == "to":
                out = canary(dev, B * cells + 64)
                rc = L.q2048_env_step_to(tb.data_ptr(), out.data_ptr(), ta.data_ptr(), tact.data_ptr(), B, n, seed, env_id0,
                                         ctr, flags, r.data_ptr(), d.data_ptr(), m.data_ptr(), tile.data_ptr(), st.data_ptr(),
                                         None)
            else:
                dp, dv = u32(dev, given[:, 0]), u32(dev, given[:, 1])
                rc = L.q2048_env_step_draws(tb.data_ptr(), ta.data_ptr(), tact.data_ptr(), dp.data_ptr(), dv.data_ptr(), B, n,
                                            r.data_ptr(), d.data_ptr(), m.data_ptr(), st.data_ptr(), None)
            assert rc == 0, what
            assert int(st.item()) == wstatus, what
            got_b = host_bytes(out)[:B * cells].reshape(B, cells)
            bad = np.flatnonzero((got_b != wb).any(axis=1))
            assert len(bad) == 0, f"{what}: boards of {len(bad)} lanes differ, first lane {bad[0]} (action {actions[bad[0]]})"
            got_a = host_bytes(ta)[:16 * B].reshape(B, 16)
            bad = np.flatnonzero((got_a != wa.view(np.uint8).reshape(B, 16)).any(axis=1))
            assert len(bad) == 0, f"{what}: aux of lane {bad[0]}: {got_a[bad[0]].view(AUX)} != {wa[bad[0]]}"
            assert np.array_equal(host_bytes(r).view(np.uint32)[:B], bits(wr)), f"{what}: reward bits"
            assert np.array_equal(host_bytes(d)[:B], wd) and np.array_equal(host_bytes(m)[:B], wm), what
            for t, k, name in ((out, B * cells, "boards"), (ta, 16 * B, "aux"), (r, B, "reward"), (d, B, "done"), (m, B, "max_log2")):
                assert_canary_beyond(t, k, f"{what} {name}")
            if entry == "to":
                assert np.array_equal(host_bytes(tile).view(np.int32)[:B], wt), f"{what}: max_tile"
                assert_canary_beyond(tile, B, f"{what} max_tile")
                assert np.array_equal(host_bytes(tb)[:B * cells].reshape(B, cells), envs["board"][:, :cells]), "boards_in was written"
                assert_canary_beyond(tb, B * cells, f"{what} boards_in")
            else:
                assert (host_bytes(tile) == CANARY).all()


def reset_masks(B):
    """(name, mask or None): NULL; all zero; one lane only at lane 0, 63 and 64; a whole wave without a masked lane
    between two waves with one; the last lane of a partial wave; mask bytes 2 and 255."""
    z = np.zeros(B, np.uint8)
    masks = [("null", None), ("zero", z.copy())]
    for lane in (0, 63, 64):
        if lane < B:
            m = z.copy()
            m[lane] = 1
            masks.append((f"lane {lane}", m))
    if B > 140:
        m = z.copy()
        m[[17, 140]] = 1
        masks.append(("waves 0 and 2", m))
    m = z.copy()
    m[B - 1] = 1
    masks.append(("last lane", m))
    m = z.copy()
    m[::3], m[1::3] = 2, 255
    masks.append(("bytes 2 and 255", m))
    return masks


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_env_reset_with_raw_masks(pkg, O, dev, n):
    """q2048_env_reset_ex: a masked lane equals the oracle's reset with the draws of (seed, its env id, its next episode,
    the reset stream), with and without Q2048_FLAG_RESET_SHAPING; every other lane, and everything beyond lane B, is
    bit-identical to before."""
    L, cells, seed = lib(pkg, dev), n * n, 21
    for B in (1, 65, 200, 257):
        env_id0 = ID_FAR if B % 2 else 0
        envs = midgame(O, n, B, seed, env_id0)
        boards, aux = envs["board"][:, :cells].copy(), aux_of(envs)
        for name, mask in reset_masks(B):
            for flags in (0, RESET_SHAPING):
                what = f"B={B} mask={name} flags={flags}"
                wb, wa = boards.copy(), aux.copy()
                for i in range(B) if mask is None else np.flatnonzero(mask):
                    e = O.Env(n)
                    e.rec[0] = envs[i]
                    e.rec["episode"][0] += 1
                    e.reset(O.draws(seed, env_id0 + int(i), int(e.rec["episode"][0]), O.STREAM_RESET))
                    if flags:
                        O.lib().orc_env_reset_shaping(e.rec.ctypes.data)
                    wb[i], wa[i] = e.board, aux_of(e.rec)[0]
                    assert wa[i]["score"] == 0 and wa[i]["ep_return"] == 0 and wa[i]["episode"] == aux[i]["episode"] + 1
                tb = torch.cat([u8(dev, boards).reshape(-1), canary(dev, 64)])
                ta = torch.cat([dev_of(dev, aux.view(np.uint8).reshape(B, 16), torch.uint8).reshape(-1), canary(dev, 64)])
                tm = None if mask is None else u8(dev, mask)
                assert L.q2048_env_reset_ex(tb.data_ptr(), ta.data_ptr(), None if tm is None else tm.data_ptr(), B, n, seed,
                                            env_id0, flags, None) == 0
                got_b, got_a = host_bytes(tb), host_bytes(ta)
                bad = np.flatnonzero((got_b[:B * cells].reshape(B, cells) != wb).any(axis=1))
                assert len(bad) == 0, f"{what}: board of lane {bad[0]}"
                bad = np.flatnonzero((got_a[:16 * B].reshape(B, 16) != wa.view(np.uint8).reshape(B, 16)).any(axis=1))
                assert len(bad) == 0, f"{what}: aux of lane {bad[0]}"
                assert (got_b[B * cells:] == CANARY).all() and (got_a[16 * B:] == CANARY).all(), f"{what}: written beyond B"


# ---------------------------------------------------------------------------------------------------------------
# 4. the two small kernels
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_rowcache_rebind_on_hand_built_records(pkg, dev, n):
    """include/q2048.h: every record without a slot that a call on `from_table` left becomes one of `to_table`; every
    other record is emptied.  Kinds, one per lane: empty; a slot under tag_from; rowless under tag_from; rowless under
    another tag; rowless under tag_from but key 0."""
    L, words = lib(pkg, dev), words_of(n)
    to_table = new_table(dev, 6)
    from_addr, from_cap, to_cap = 0x7F0012340000, 14, 6
    tag_from, tag_to = M.cache_tag(from_addr, from_cap), M.cache_tag(to_table.data_ptr(), to_cap)
    tag_else = M.cache_tag(from_addr, from_cap + 1)
    assert len({tag_from, tag_to, tag_else}) == 3
    for B in (1, 64, 65, 257):
        rng = np.random.default_rng(B + n)
        lane = np.arange(B + 8)
        kind = (lane + (B == 1) * 2) % 5
        keys, q = M.random_rows(rng, len(lane), words)
        rec = M.pack_records(n, keys, q, np.where(kind == 1, lane % 1000, M.ROWLESS), tag_from)
        rec[kind == 0] = np.zeros(1, M.RECORD[n])
        rec["slot"][kind == 3] = U(M.ROWLESS | tag_else)
        rec["key"][kind == 4] = 0
        want = rec.copy()
        keep = (kind == 2)[:B]
        want[:B][~keep] = np.zeros(1, M.RECORD[n])
        want["slot"][:B][keep] = U(M.ROWLESS | tag_to)
        cache = cache_of(dev, rec[:B], extra=8)
        want_bytes = np.concatenate([want[:B].view(np.uint8).reshape(-1), np.full(8 * M.RECORD[n].itemsize, CANARY, np.uint8)])
        assert L.q2048_rowcache_rebind(cache.data_ptr(), B, n, from_addr, from_cap, to_table.data_ptr(), to_cap, None) == 0
        got = host_bytes(cache)
        bad = np.flatnonzero(got != want_bytes)
        assert len(bad) == 0, f"B={B}: byte {bad[0]} (record {bad[0] // M.RECORD[n].itemsize}, kind {kind[bad[0] // M.RECORD[n].itemsize]})"
        assert not raw(to_table).any()


@pytest.mark.parametrize("dev", DEVICES)
def test_encode_onehot_on_written_boards(pkg, dev):
    """q2048_encode_onehot for B = 1 (a quarter of a block), 3, 5 (a block and a quarter) and 1000: out[i][c][r][col] = 1
    iff the byte at (r, col) equals c.  The boards carry every value 0..15 in every cell, and 16, 17 and 255, which
    encode as all zeros.  float32 compared as bits, bfloat16 as uint16 (0x3F80 / 0); a canary behind the last byte."""
    L = lib(pkg, dev)
    values = np.array(list(range(16)) + [16, 17, 255], dtype=np.uint8)
    for B in (1, 3, 5, 1000):
        i = np.arange(B)[:, None]
        boards = values[(i * 3 + np.arange(16)[None, :] * (1 + i % 5) + i // 19) % len(values)]
        if B == 1000:
            for cell in range(16):
                assert set(boards[:, cell].tolist()) == set(values.tolist())
        tb = u8(dev, boards)
        hot = boards[:, None, :] == np.arange(16, dtype=np.uint8)[None, :, None]         # [B, 16 channels, 16 cells]
        for dtype, one, width in ((0, np.uint32(0x3F800000), np.uint32), (1, np.uint16(0x3F80), np.uint16)):
            out = canary(dev, B * 256 * np.dtype(width).itemsize + 64)
            assert L.q2048_encode_onehot(tb.data_ptr(), B, dtype, out.data_ptr(), None) == 0
            got = host_bytes(out)
            body = got[:B * 256 * np.dtype(width).itemsize].view(width).reshape(B, 16, 16)
            assert np.array_equal(body, np.where(hot, one, width(0))), f"B={B} dtype={dtype}"
            assert (got[B * 256 * np.dtype(width).itemsize:] == CANARY).all(), f"B={B} dtype={dtype}: written beyond the last board"
        assert np.array_equal(tb.cpu().numpy(), boards)
