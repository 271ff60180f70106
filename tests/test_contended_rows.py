"""What the Q-table kernels leave behind when lanes SHARE a row: crowds on one (s, a), lanes that create one row at
the same time, and 5x5 keys that share their first word.

Everywhere else in the suite the keys of two lanes are disjoint (tests/test_four_call_kernels.py::model_update says so
in its first line), so the claim's lost compare-and-swap, the wait for a 5x5 key's second word and the retry branch of
`td_update` run there only under property checks at workload sizes.  Here they run on a handful of lanes, and what is
asserted is exact -- integers and float32 bit patterns, no tolerance -- and follows from atomicity alone:

  f(q) = M.td_value(q, r, 0, ...) where the bootstrap term is zero (done = 1, or an s' whose row is absent or fresh);
  a CROWD is K lanes with the same s, the same action index `a` into the stored row and the same reward bits;
  the CHAIN is c_k = f^k(q0), q0 the entry's value before the call (0 for an absent row).

  store mode        the entry ends as some c_k, 1 <= k <= K: every written value is f of a value the entry held
                    earlier.  A torn value, a value from a wrong row or a write into a duplicate row lie outside it.
  strict, K <= 16   (Q2048_FLAG_TD_CAS) the entry ends as exactly c_K and CAS_FALLBACK does not move: a swap fails only
                    because another lane wrote in between, each other lane writes once, so a lane fails at most
                    K - 1 <= 15 times; the chain's values are distinct, so a changed value never returns (no ABA).
  strict, any K     the entry ends in the chain, and 16 * fallbacks <= retries <= 16 * K (a lane falls back after
                    exactly 16 failures).
  device, strict,   retries >= K - 1: the K lanes of one wave have all read the same bits before the wave's first swap
  one wave          issues, and exactly one of them succeeds.  (This is what proves that the retry branch ran.)
  keys, every mode  one row per distinct key the call touches: INSERTS is the number of distinct keys that were absent,
                    `check_structure` holds within the learning paths' probe limit, DROPS is 0, the status is the
                    filler lanes' own, q2048_claim_timeouts is 0, the other three values of the row of s and every row
                    the call did not address keep their bits.

Each case asserts from the model that its chain has K + 1 distinct members (lr = 0.1 reaches its float32 fixed point
near k = 143, so the 1025-lane crowd takes lr = 0.001), and each strict case that c_K != c_1, so strict and default mode
cannot pass the same check.  Every test ends by showing that its checks can fail: the chain run K - 1 steps does not
match a strict result, a value one ulp off the chain is refused, and an image with one duplicated key is refused by
`check_structure`.

Tables and caches are raw bytes written and read through tests/table_model.py; the entry points are called through
ctypes with the helpers of tests/test_four_call_kernels.py.  Every test runs on the CPU twin and on the GPU.  On the twin
a crowd below 2049 lanes is one thread, so there the same assertions hold of a sequential schedule; the cases with
B >= 4097 run three twin threads.  Each case prints what it observed (CAS_RETRY, CAS_FALLBACK, the chain depth k the
entry ended at): observations for whoever touches `td_update` or the claim next, not thresholds."""
import numpy as np
import pytest
import torch

import table_model as M
import test_four_call_kernels as FC
import test_symmetric_table as ST
from table_model import U
from test_four_call_kernels import (DEVICES, assert_records, assert_rows_equal_dict, call_update, fresh_cache, key_tuples,
                                    lib, new_table, raw, rows_dict, words_of)

BAD_ACTION = 1
INDEPENDENT, TD_CAS, SYMMETRIC = 1, 4, 1 << 26
ST_STEPS, ST_EPISODES, ST_VALID, ST_INSERTS, ST_DROPS, ST_EXPLORE, ST_CAS_RETRY, ST_CAS_FALLBACK, NSTAT = 0, 1, 2, 4, 5, 6, 7, 31, 32
SF_REWARD = 2
MAX_CAS = 16
WAVE = 64


# ---------------------------------------------------------------------------------------------------------------
# the chain and its checks
# ---------------------------------------------------------------------------------------------------------------
def b32(x):
    return int(np.float32(x).view(np.uint32))


def chain_of(q0, reward, lr, gamma, K):
    """[c_0 .. c_K] with c_k = f^k(q0); asserts that the K + 1 members have distinct bits."""
    c = [np.float32(q0)]
    for _ in range(K):
        c.append(M.td_value(c[-1], reward, 0.0, True, lr, gamma))
    assert len({b32(x) for x in c}) == K + 1, f"the chain from {q0} to {reward} at lr={lr} is not distinct over {K} steps"
    # (done or not: with a zero bootstrap the target is the reward either way)
    assert b32(M.td_value(c[0], reward, 0.0, False, lr, gamma)) == b32(c[1])
    return c


def check_entry(got_bits, chain, K, strict, what):
    """The entry's bits after a crowd of K lanes -> the depth k with c_k == entry.  Store mode and strict mode beyond 16
    lanes: 1 <= k <= K.  Strict mode up to 16 lanes: k == K."""
    where = {b32(x): k for k, x in enumerate(chain[:K + 1])}
    k = where.get(int(got_bits))
    assert k is not None and k >= 1, (f"{what}: the entry holds {int(got_bits):#010x}, which is none of c_1 .. c_{K} "
                                      f"(c_0 = {b32(chain[0]):#010x}, c_1 = {b32(chain[1]):#010x}, c_K = {b32(chain[K]):#010x})")
    if strict and K <= MAX_CAS:
        assert k == K, f"{what}: strict mode with {K} lanes left c_{k}, not c_{K}: an update was lost"
    return k


def check_counters(dev, retries, fallbacks, K, strict, one_wave, what, entries=1):
    """CAS_RETRY and CAS_FALLBACK of a call whose only shared entries are `entries` crowds of K lanes each."""
    if not strict:
        assert retries == 0 and fallbacks == 0, f"{what}: store mode moved the CAS counters by {retries}, {fallbacks}"
        return
    assert MAX_CAS * fallbacks <= retries <= MAX_CAS * K * entries, f"{what}: retries={retries} fallbacks={fallbacks}"
    if K <= MAX_CAS:
        assert fallbacks == 0, f"{what}: {fallbacks} fallbacks with only {K} lanes on the entry"
    if dev != "cpu" and one_wave:
        assert retries >= (K - 1) * entries, f"{what}: {retries} retries, a wave of {K} lanes on one entry owes {K - 1}"


def assert_teeth(got_bits, chain, K, strict, after, words):
    """The checks above can fail."""
    if strict and K <= MAX_CAS and K >= 2:
        with pytest.raises(AssertionError, match="none of c_1"):
            check_entry(got_bits, chain[:K], K - 1, True, "teeth")          # the model run with K - 1 steps
        with pytest.raises(AssertionError, match="an update was lost"):
            check_entry(b32(chain[K - 1]), chain, K, True, "teeth")         # one update short of the chain's end
        assert b32(chain[K]) != b32(chain[1])
    with pytest.raises(AssertionError, match="none of"):
        check_entry(int(got_bits) ^ 1, chain, K, strict, "teeth")           # one ulp off the chain
    occ = np.flatnonzero(after[:, 0] != 0)
    hole = int(np.flatnonzero(after[:, 0] == 0)[0])
    bad = after.copy()
    bad[hole] = after[occ[0]]                                               # one duplicated key
    with pytest.raises(AssertionError, match="occurs again"):
        M.check_structure(bad, words, M.ROLLOUT_PROBE)


def entry_bits(image, key, a, words):
    at = M.find_slot(image, key, words)
    assert at >= 0, f"the row of key {[hex(w) for w in key]} is not in the table"
    return int(np.ascontiguousarray(image[at, 1:3]).view(np.uint32)[a])


def observed(dev, what, retries, fallbacks, k, K):
    print(f"OBSERVED [{dev}] {what}: CAS_RETRY +{retries}, CAS_FALLBACK +{fallbacks}, entry = c_{k} of K = {K}")


def one_wave(lanes, block):
    lanes = np.asarray(lanes)
    return len(set((lanes // WAVE).tolist())) == 1 and len(set((lanes // block).tolist())) == 1


# ---------------------------------------------------------------------------------------------------------------
# 1. q2048_q_update / q2048_q_update_cached: a crowd among private filler lanes
# ---------------------------------------------------------------------------------------------------------------
# name: (B, the crowd's lanes, lr).  The update kernel's workgroup is 1024 lanes.
CROWDS = {
    "wave2": (130, [67, 101], 0.1),                                          # inside one wave
    "wave16": (130, list(range(64, 128, 4)), 0.1),
    "wave17": (130, list(range(64, 115, 3)), 0.1),                           # one lane more than strict mode's bound
    "wave64": (200, list(range(64, 128)), 0.1),
    "block16": (1100, [64 * w + (5 * w) % 64 for w in range(16)], 0.1),      # one lane in each wave of one workgroup
    "blocks5": (4100, [0, 1024, 2048, 3072, 4096], 0.1),                     # one lane in each of five workgroups
    "big1025": (4200, list(range(50, 50 + 4 * 1025, 4)), 0.001),             # across workgroups and twin threads
}
CROWD_ACTION, CROWD_REWARD = 2, np.float32(2.5)
CROWD_ROW = np.array([0.75, -0.5, -1.25, 0.5], dtype=np.float32)             # the row of s where it is written beforehand
_CROWD_WORLDS = {}


def crowd_world(n, name):
    """The call's inputs: FC.transitions for every lane (pairwise-disjoint keys), then the crowd's lanes overwritten
    with ONE s, action, reward and done = 1, and s' drawn from three boards -- at 4x4 s and the three s' share a home
    slot, so the claims of several keys meet in one slot.  No filler lane touches a crowd key."""
    if (n, name) not in _CROWD_WORLDS:
        B, lanes, lr = CROWDS[name]
        lanes, words = np.array(lanes), words_of(n)
        K = len(lanes)
        assert len(set(lanes.tolist())) == K and lanes.max() < B
        t = FC.transitions(n, B, False, seed=4000 * n + B)
        ks, kn = FC.lane_keys(t, n, 0)                                       # (asserts that no two lanes touch one key)
        crowd = np.zeros(B, bool)
        crowd[lanes] = True
        rng = np.random.default_rng(17 * n + B)
        cap_log2 = t["cap_log2"]
        if n == 4:
            home = int(rng.integers(0, 1 << cap_log2))
            cells = M.cells_of_key4(M.keys_with_home(rng, cap_log2, 1, [home] * 4))
        else:
            cells = FC.random_boards(rng, 4, n)
        t["s"][lanes] = cells[0]
        t["s2"][lanes] = cells[1 + np.arange(K) % 3]
        t["actions"][lanes], t["done"][lanes] = CROWD_ACTION, 1
        t["reward"] = t["reward"].copy()
        t["reward"][lanes] = CROWD_REWARD
        t["s_there"][lanes] = t["n_there"][lanes] = t["same"][lanes] = False
        key_s = key_tuples(M.state_key(cells[:1], n), n)[0]
        next_of = key_tuples(M.state_key(t["s2"][lanes], n), n)
        fill = np.flatnonzero(~crowd)
        filler_keys = {ks[i] for i in fill} | {kn[i] for i in fill}
        crowd_keys = {key_s} | set(next_of)
        assert len(crowd_keys) == 1 + min(3, K) and not filler_keys & crowd_keys, "a filler lane touches a crowd key"
        keys = [ks[i] for i in fill if t["s_there"][i]] + [kn[i] for i in fill if t["n_there"][i]]
        q = np.concatenate([t["q_s"][~crowd & t["s_there"]], t["q_n"][~crowd & t["n_there"]]]).reshape(-1, 4)
        images = {False: M.build_image(cap_log2, np.array(keys, dtype=U).reshape(-1, words), q, words),
                  True: M.build_image(cap_log2, np.array(keys + [key_s], dtype=U).reshape(-1, words),
                                      np.concatenate([q, CROWD_ROW[None]]), words)}
        _CROWD_WORLDS[n, name] = dict(t=t, B=B, lanes=lanes, K=K, lr=lr, fill=fill, ks=ks, kn=kn, key_s=key_s,
                                      next_of=next_of, images=images, cap_log2=cap_log2)
    return _CROWD_WORLDS[n, name]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("name", list(CROWDS))
def test_update_crowd(pkg, dev, n, name):
    """q2048_q_update and _cached, default and strict mode, the row of s absent (the crowd creates it) or written
    beforehand: the filler lanes against the sequential model, the crowd's entry against the chain, one zero row per
    distinct s', every other bit as it was, and with a cache every crowd lane's record = the key of its s', the zero
    row, the slot that key lies in, the table's tag."""
    L, words, gamma = lib(pkg, dev), words_of(n), 0.9
    w = crowd_world(n, name)
    t, B, K, lr, fill, key_s, a = w["t"], w["B"], w["K"], w["lr"], w["fill"], w["key_s"], CROWD_ACTION
    flip = list(CROWDS).index(name) % 2 == 1                                 # every combination over the list of cases
    for flags, present, cached in ((0, flip, False), (0, not flip, True), (TD_CAS, flip, True), (TD_CAS, not flip, False)):
        what = f"{name} n={n} flags={flags} s {'present' if present else 'absent'} cached={cached}"
        strict, image = bool(flags & TD_CAS), w["images"][present]
        M.check_structure(image, words, M.ROLLOUT_PROBE)
        d = rows_dict(image, n)
        status, inserts, drops, left_f = FC.model_update(d, [w["ks"][i] for i in fill], [w["kn"][i] for i in fill],
                                                         t["actions"][fill], t["reward"][fill], t["done"][fill], lr, gamma, flags)
        assert (key_s in d) == present and drops == 0
        if not present:
            d[key_s] = np.zeros(4, np.float32)
        for k in set(w["next_of"]):
            assert k not in d
            d[k] = np.zeros(4, np.float32)
        inserts += (not present) + len(set(w["next_of"]))
        chain = chain_of(d[key_s][a], CROWD_REWARD, lr, gamma, K)
        left = [None] * B
        for i, rec in zip(fill, left_f):
            left[i] = rec
        for i, k in zip(w["lanes"], w["next_of"]):
            left[i] = (k, np.zeros(4, np.float32), True)

        table = new_table(dev, w["cap_log2"], image)
        cache = fresh_cache(dev, n, B) if cached else None
        before = FC.host_bytes(cache).reshape(-1, M.RECORD[n].itemsize) if cached else None
        delta, got_status = call_update(L, dev, table, w["cap_log2"], t, n, lr, gamma, 0, flags, cache)
        after = raw(table)

        assert got_status == status, f"{what}: status {got_status}, the filler lanes' is {status}"
        got = entry_bits(after, key_s, a, words)
        depth = check_entry(got, chain, K, strict, what)
        observed(dev, what, int(delta[ST_CAS_RETRY]), int(delta[ST_CAS_FALLBACK]), depth, K)
        check_counters(dev, int(delta[ST_CAS_RETRY]), int(delta[ST_CAS_FALLBACK]), K, strict, one_wave(w["lanes"], 1024), what)
        want = np.zeros(NSTAT, np.int64)
        want[ST_INSERTS], want[ST_CAS_RETRY], want[ST_CAS_FALLBACK] = inserts, delta[ST_CAS_RETRY], delta[ST_CAS_FALLBACK]
        assert np.array_equal(delta, want), f"{what}: statistics moved by {delta.tolist()}, expected inserts={inserts} and no drops"
        d[key_s][a] = np.array([got], dtype=np.uint32).view(np.float32)[0]
        assert_rows_equal_dict(after, d, n, what)                            # (one row per key, every other value kept)
        M.check_structure(after, words, M.ROLLOUT_PROBE)
        if cached:
            assert_records(n, cache, left, before, after, M.cache_tag(table.data_ptr(), w["cap_log2"]), False, what)
        assert_teeth(got, chain, K, strict, after, words)
    assert pkg._native.claim_timeouts(L) == 0


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("name", ["wave17", "block16", "blocks5"])
def test_update_crowd_vanishes_with_private_rows(pkg, dev, n, name):
    """The same inputs with Q2048_FLAG_INDEPENDENT (and strict mode): the keys carry the lane's salt, so the crowd is K
    private rows for s, each exactly c_1 from zero, the written row of the unsalted s keeps its bits, and no swap is
    ever retried.  The whole call is the sequential model's."""
    L, words, gamma = lib(pkg, dev), words_of(n), 0.9
    w = crowd_world(n, name)
    t, B, K, lr, a = dict(w["t"], independent=True), w["B"], w["K"], w["lr"], CROWD_ACTION
    ks, kn = FC.lane_keys(t, n, FC.ID_FAR)                                   # (asserts: no two lanes touch one key)
    image = w["images"][True]
    d = rows_dict(image, n)
    status, inserts, drops, _ = FC.model_update(d, ks, kn, t["actions"], t["reward"], t["done"], lr, gamma, TD_CAS)
    c1 = chain_of(0.0, CROWD_REWARD, lr, gamma, 1)[1]
    rows_s = {ks[i] for i in w["lanes"]}
    assert len(rows_s) == K and all(b32(d[k][a]) == b32(c1) for k in rows_s)
    table = new_table(dev, w["cap_log2"], image)
    delta, got_status = call_update(L, dev, table, w["cap_log2"], t, n, lr, gamma, FC.ID_FAR, INDEPENDENT | TD_CAS)
    after = raw(table)
    assert got_status == status
    FC.assert_stats(delta, inserts, drops, f"{name} private rows")            # (every other statistic 0: no retry)
    assert_rows_equal_dict(after, d, n, f"{name} private rows")
    M.check_structure(after, words, M.ROLLOUT_PROBE)
    assert np.array_equal(after[M.find_slot(after, w["key_s"], words)], image[M.find_slot(image, w["key_s"], words)])
    assert pkg._native.claim_timeouts(L) == 0


# ---------------------------------------------------------------------------------------------------------------
# 2. 5x5 keys that share their first word
# ---------------------------------------------------------------------------------------------------------------
SHARED_LANES = np.concatenate([np.arange(9), 64 + np.arange(9), 1024 + np.arange(9)])   # one wave, a second, a second workgroup
SHARED_B = 1033
SHARED_REWARD = np.array([1.5, -0.75, 3.25], dtype=np.float32)
SHARED_ROW = np.array([0.5, -0.5, 0.25, -0.25], dtype=np.float32)
_SHARED = {}


def shared_word_world(cap_log2, prewritten):
    """Three 5x5 boards whose cells 0..11 and the low three bits of cell 12 are equal -- one first key word, three second
    words -- and whose homes lie in ONE 128-byte line, found by search with the model; that line is filled by rows of
    other keys (each at its own home) but for one slot `empty`.  `prewritten`: the first of the three is written as
    well (where `build_image` puts it: on the other two's sequences, they enter the same line), leaving one empty slot
    again.  Every absent key's sequence therefore ends at `empty`: that is the slot the model predicts the first-word
    compare-and-swap is raced for, and lost at by all keys but one."""
    if (cap_log2, prewritten) not in _SHARED:
        mask = (1 << cap_log2) - 1
        for seed in range(50):
            rng = np.random.default_rng(1000 * cap_log2 + seed)
            boards = np.repeat(rng.integers(0, 18, size=(1, 25)).astype(np.uint8), 100, axis=0)
            boards[:, 0] |= 1
            boards[:, 13:] = rng.integers(0, 18, size=(100, 12))
            boards[:, 12] = (boards[0, 12] & 7) | (rng.integers(0, 2, size=100) << 3)
            boards = np.unique(boards, axis=0)
            keys = M.state_key(boards, 5)
            assert (keys[:, 0] == keys[0, 0]).all() and len(np.unique(keys[:, 1])) == len(keys)
            line = ((M.key_hash(keys, 2) & U(mask)) >> U(2)).astype(np.int64)
            full = np.flatnonzero(np.bincount(line) >= 3)
            if len(full):
                break
        else:
            raise AssertionError("no three keys with one home line in 50 x 100 draws")
        home_line = int(full[0])
        trio = boards[np.flatnonzero(line == home_line)[:3]]
        tk = M.state_key(trio, 5)
        slots = [4 * home_line + j for j in range(4)]
        rng = np.random.default_rng(cap_log2)
        other = M.keys_with_home(rng, cap_log2, 2, slots[1:3] if prewritten else slots[1:])
        assert not (other[:, 0] == tk[0, 0]).any()
        keys = np.concatenate([other, tk[:1]]) if prewritten else other
        q = np.concatenate([rng.standard_normal((len(other), 4)).astype(np.float32), SHARED_ROW[None]])[:len(keys)]
        image = M.build_image(cap_log2, keys, q, 2)
        M.check_structure(image, 2, M.ROLLOUT_PROBE)
        empty = [s for s in slots if image[s, 0] == 0]
        assert len(empty) == 1
        h = M.key_hash(tk, 2)
        if prewritten:
            at = M.find_slot(image, tuple(int(x) for x in tk[0]), 2)
            assert at in slots and (M.pos_of(h[1:], cap_log2, at) < 4).all()          # on the others' sequences
        # every absent key of the three meets only occupied slots before `empty`
        for r in range(1 if prewritten else 0, 3):
            p = int(M.pos_of(h[r], cap_log2, empty[0]))
            assert p < 4 and all(image[int(M.slot_at(h[r], cap_log2, j)), 0] != 0 for j in range(p))
        _SHARED[cap_log2, prewritten] = dict(trio=trio, keys=key_tuples(tk, 5), image=image, empty=empty[0])
    return _SHARED[cap_log2, prewritten]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("cap_log2", [4, 6, 10])
@pytest.mark.parametrize("prewritten", [False, True])
def test_5x5_keys_with_one_first_word(pkg, dev, cap_log2, prewritten):
    """Nine lanes per key in one call (three in a wave, three in another, three in a second workgroup), lane j asks for
    key j % 3 as s and for key (j + 1) % 3 as s', done = 1; every other lane has a bad action and does nothing.

    All absent: the three keys' sequences end at the one empty slot of their home line (`empty` of the world above).
    The model predicts that the claim's compare-and-swap on the first word is raced there by lanes with three second
    words: one key wins it, a lane of another key finds the first word equal (`confirm` with won == false), reads the
    owner's second word -- waiting for it if need be -- finds hi != key.k1 and goes on to the next line, where the two
    remaining keys settle the same way.  Pre-written: one key's row is in the table, with values, in that line; its
    lanes must find THAT row (their chain starts at its value and ends in its entry) while the other two are created.
    Expected: one row per key, each under its own second word, each entry the end of its own chain; nothing else."""
    L, n, words, lr, gamma = lib(pkg, dev), 5, 2, 0.1, 0.9
    w = shared_word_world(cap_log2, prewritten)
    which = np.arange(len(SHARED_LANES)) % 3
    K = 9
    boards = np.repeat(w["trio"][:1], SHARED_B, axis=0)
    t = dict(s=boards.copy(), s2=boards.copy(), actions=np.full(SHARED_B, 255, np.uint8),
             reward=np.zeros(SHARED_B, np.float32), done=np.ones(SHARED_B, np.uint8))
    t["s"][SHARED_LANES], t["s2"][SHARED_LANES] = w["trio"][which], w["trio"][(which + 1) % 3]
    t["actions"][SHARED_LANES], t["reward"][SHARED_LANES] = (which + 1) % 4, SHARED_REWARD[which]
    for flags in (0, TD_CAS):
        what = f"2^{cap_log2} slots prewritten={prewritten} flags={flags}"
        strict, d = bool(flags & TD_CAS), rows_dict(w["image"], n)
        assert [k in d for k in w["keys"]] == [prewritten, False, False]
        for k in w["keys"]:
            d.setdefault(k, np.zeros(4, np.float32))
        chains = [chain_of(d[k][(r + 1) % 4], SHARED_REWARD[r], lr, gamma, K) for r, k in enumerate(w["keys"])]
        table = new_table(dev, cap_log2, w["image"])
        delta, status = call_update(L, dev, table, cap_log2, t, n, lr, gamma, 0, flags)
        after = raw(table)
        assert status == BAD_ACTION
        retries, fallbacks = int(delta[ST_CAS_RETRY]), int(delta[ST_CAS_FALLBACK])
        check_counters(dev, retries, fallbacks, K, strict, False, what, entries=3)
        for r, k in enumerate(w["keys"]):
            got = entry_bits(after, k, (r + 1) % 4, words)
            depth = check_entry(got, chains[r], K, strict, f"{what} key {r}")
            observed(dev, f"{what} key {r}", retries, fallbacks, depth, K)
            d[k][(r + 1) % 4] = np.array([got], dtype=np.uint32).view(np.float32)[0]
        want = np.zeros(NSTAT, np.int64)
        want[ST_INSERTS], want[ST_CAS_RETRY], want[ST_CAS_FALLBACK] = 3 - prewritten, retries, fallbacks
        assert np.array_equal(delta, want), f"{what}: statistics moved by {delta.tolist()}"
        assert_rows_equal_dict(after, d, n, what)
        M.check_structure(after, words, M.ROLLOUT_PROBE)
        assert after[w["empty"], 0] == U(w["keys"][0][0]), f"{what}: the raced slot {w['empty']} holds none of the three keys"
        assert_teeth(got, chains[2], K, strict, after, words)
    assert pkg._native.claim_timeouts(L) == 0


# ---------------------------------------------------------------------------------------------------------------
# 3. one fused step on a crowd
# ---------------------------------------------------------------------------------------------------------------
FUSED = {                                                                    # name: (B, the crowd's lanes)
    "wave8": (8, list(range(8))),
    "wave64": (64, list(range(64))),
    # one lane in each of sixteen consecutive waves: the fused workgroup is 256 lanes, so this is every wave of four
    # workgroups; the other lanes are filler envs on boards of their own
    "waves16": (1064, [64 * w + (7 * w) % 64 for w in range(16)]),
}
FUSED_SEED, FUSED_CTR = 31, 50
_FUSED = {}


def step_model(O, envs, actions, n):
    """One oracle step per lane on its own spawn draws -> boards, aux, reward, done, keys before and after, valid."""
    B, cells = len(envs), n * n
    aux = FC.aux_of(envs)
    x = np.array([O.draws(FUSED_SEED, i, FUSED_CTR) for i in range(B)], dtype=np.uint32)
    boards, out_aux, reward, done, _, _, status = FC.model_step(O, envs, aux, actions, n, x[:, 2:], x[:, :2], False)
    assert status == 0
    before = envs["board"][:, :cells].copy()
    return dict(before=before, aux=aux, boards=boards, out_aux=out_aux, reward=reward, done=done,
                valid=(boards != before).any(axis=1))


def valid_moves(O, board, n):
    return [a for a in range(4) if O.move(board, a, n)[2]]


def fused_world(O, n, name):
    """K lanes hold ONE board and ONE aux record (an oracle env after random play), the other lanes envs of their own.
    The table holds only the row of the crowd's board, written so that its greedy action `a` is a valid move and stays
    the greedy one along the whole chain.  Found by search over seeds of the random play; asserted from the oracle: no
    lane's episode ends, the crowd's rewards have the same bits, and no filler lane touches a key of another lane."""
    if (n, name) not in _FUSED:
        B, lanes = FUSED[name]
        lanes = np.array(lanes)
        crowd = np.zeros(B, bool)
        crowd[lanes] = True
        for seed in range(FUSED_SEED, FUSED_SEED + 20):
            envs = O.envs_init(B, n, seed, 0)
            O.rollout(envs, None, 40, seed, 0, 0)
            moves = [a for a in valid_moves(O, envs["board"][lanes[0], :n * n], n) if a != 0]
            if not moves:
                continue
            envs[lanes] = envs[lanes[0]]
            actions = np.where(crowd, moves[0], 0).astype(np.uint8)
            m = step_model(O, envs, actions, n)
            ks, kn = key_tuples(M.state_key(m["before"], n), n), key_tuples(M.state_key(m["boards"], n), n)
            crowd_keys = {ks[lanes[0]]} | {kn[i] for i in lanes}
            touched = [k for i in np.flatnonzero(~crowd) for k in {ks[i], kn[i]}]
            if (not m["done"].any() and len({b32(r) for r in m["reward"][lanes]}) == 1 and m["valid"][lanes].all()
                    and len(set(touched)) == len(touched) and not set(touched) & crowd_keys):
                break
        else:
            raise AssertionError("no seed met the preconditions")
        r = m["reward"][lanes[0]]
        row = np.float32(r) - np.float32(1.0) - np.float32(0.25) * np.arange(4, dtype=np.float32)
        row[moves[0]] = np.float32(r) + np.float32(1.0)
        _FUSED[n, name] = dict(B=B, lanes=lanes, crowd=crowd, envs=envs, a=moves[0], m=m, ks=ks, kn=kn, row=row, reward=r)
    return _FUSED[n, name]


def call_fused(L, dev, table, cap_log2, boards, aux, n, lr, gamma, flags):
    B = len(boards)
    tb = FC.u8(dev, boards)
    ta = FC.dev_of(dev, aux.view(np.uint8).reshape(B, 16), torch.uint8)
    si0 = np.arange(100, 100 + NSTAT, dtype=np.int64)
    si, sf = torch.from_numpy(si0.copy()).to(dev), torch.zeros(4, dtype=torch.float64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    assert L.q2048_fused_rollout(tb.data_ptr(), ta.data_ptr(), table.data_ptr(), cap_log2, B, n, 1, 0.0, lr, gamma,
                                 FUSED_SEED, 0, FUSED_CTR, flags, si.data_ptr(), sf.data_ptr(), st.data_ptr(), None) == 0
    return (FC.host_bytes(tb).reshape(B, n * n), FC.host_bytes(ta).reshape(B, 16), si.cpu().numpy() - si0,
            sf.cpu().numpy(), int(st.item()))


def assert_fused_outputs(got, m, B, inserts, strict, what):
    """Boards and aux as the oracle left them, the statistics of one step without an episode's end."""
    boards, aux, delta, sf, status = got
    assert status == 0, f"{what}: status {status}"
    assert np.array_equal(boards, m["boards"]), f"{what}: boards"
    assert np.array_equal(aux, m["out_aux"].view(np.uint8).reshape(B, 16)), f"{what}: aux"
    want = np.zeros(NSTAT, np.int64)
    want[ST_STEPS], want[ST_VALID], want[ST_INSERTS] = B, int(m["valid"].sum()), inserts
    want[ST_CAS_RETRY], want[ST_CAS_FALLBACK] = delta[ST_CAS_RETRY], delta[ST_CAS_FALLBACK]
    assert np.array_equal(delta, want), f"{what}: statistics moved by {delta.tolist()}, expected {want.tolist()}"
    assert sf[0] == 0.0 and sf[1] == 0.0 and np.isclose(sf[SF_REWARD], m["reward"].astype(np.float64).sum(), rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("name", list(FUSED))
def test_fused_step_crowd(pkg, O, dev, n, name):
    """q2048_fused_rollout, steps = 1, eps = 0, default and strict mode: every s' is absent, so each crowd lane's target
    is its reward and the entry (s, a) runs down the chain; one zero row per distinct s' (the set comes from the
    oracle: the lanes' spawn draws differ); a filler env creates the row of its own board, writes f(0) into entry 0 --
    the greedy action of a zero row, valid or not -- and creates its s' when the move was valid."""
    L, words, lr, gamma, cap_log2 = lib(pkg, dev), words_of(n), 0.1, 0.9, 12
    w = fused_world(O, n, name)
    B, lanes, m, a, K = w["B"], w["lanes"], w["m"], w["a"], len(w["lanes"])
    key_s = w["ks"][lanes[0]]
    image = M.build_image(cap_log2, np.array([key_s], dtype=U).reshape(-1, words), w["row"][None], words)
    chain = chain_of(w["row"][a], w["reward"], lr, gamma, K)
    next_keys = {w["kn"][i] for i in lanes}
    print(f"{name} n={n}: {len(next_keys)} distinct s' among {K} lanes")
    for flags in (0, TD_CAS):
        what, strict = f"fused {name} n={n} flags={flags}", bool(flags & TD_CAS)
        d = {key_s: w["row"].copy()}
        for k in next_keys:
            d[k] = np.zeros(4, np.float32)
        inserts = len(next_keys)
        for i in np.flatnonzero(~w["crowd"]):
            d[w["ks"][i]] = np.zeros(4, np.float32)
            d[w["ks"][i]][0] = M.td_value(0.0, m["reward"][i], 0.0, False, lr, gamma)
            if m["valid"][i]:
                d[w["kn"][i]] = np.zeros(4, np.float32)
            inserts += 1 + int(m["valid"][i])
        table = new_table(dev, cap_log2, image)
        got = call_fused(L, dev, table, cap_log2, m["before"], m["aux"], n, lr, gamma, flags)
        after = raw(table)
        assert_fused_outputs(got, m, B, inserts, strict, what)
        retries, fallbacks = int(got[2][ST_CAS_RETRY]), int(got[2][ST_CAS_FALLBACK])
        bits = entry_bits(after, key_s, a, words)
        depth = check_entry(bits, chain, K, strict, what)
        observed(dev, what, retries, fallbacks, depth, K)
        check_counters(dev, retries, fallbacks, K, strict, one_wave(lanes, 256), what)
        d[key_s][a] = np.array([bits], dtype=np.uint32).view(np.float32)[0]
        assert_rows_equal_dict(after, d, n, what)
        M.check_structure(after, words, M.ROLLOUT_PROBE)
        assert_teeth(bits, chain, K, strict, after, words)
    assert pkg._native.claim_timeouts(L) == 0


def symmetric_world(O, pairs):
    """Eight lanes hold the eight images of one board without a stabiliser (an oracle env after random play, its
    consecutive-action state cleared so that the reward does not depend on the env's own action index).
    pairs False: a canonical row with one maximum, at a canonical action that is a valid move: every lane's greedy env
    action maps to it.  pairs True: a canonical row of four equal values: every lane takes env action 0, the first
    maximum, which is canonical action pi_g(0) -- each of the four canonical actions for two of the eight images."""
    if ("sym", pairs) not in _FUSED:
        for seed in range(FUSED_SEED, FUSED_SEED + 40):
            envs = O.envs_init(8, 4, seed, 0)
            O.rollout(envs, None, 40, seed, 0, 0)
            base = envs["board"][0, :16].copy()
            imgs = np.stack([x.reshape(16) for x in (i[0] for i in ST.images(base.reshape(1, 4, 4)))])
            canon_board, g, ckeys = ST.canon(imgs)
            if len(np.unique(imgs, axis=0)) != 8 or len(valid_moves(O, base, 4)) != 4 or (imgs >= 16).any():
                continue
            envs[:] = envs[0]
            envs["board"][:, :16] = imgs
            envs["consecutive_action"], envs["consecutive_count"], envs["last_consecutive_penalty"] = -1, 0, 0.0
            assert len(set(ckeys.tolist())) == 1
            ac = 1                                                           # (every canonical move is valid as well)
            env_action = np.array([[e for e in range(4) if ST.pi(g[i], e) == (ST.pi(g[i], 0) if pairs else ac)][0]
                                   for i in range(8)], dtype=np.uint8)
            m = step_model(O, envs, env_action, 4)
            canon_action = ST.pi(g, env_action)
            same_reward = all(len({b32(r) for r in m["reward"][canon_action == c]}) == 1 for c in set(canon_action.tolist()))
            if not m["done"].any() and m["valid"].all() and same_reward:
                break
        else:
            raise AssertionError("no seed met the preconditions")
        top = np.float32(m["reward"].max()) + np.float32(1.0)
        if pairs:
            row = np.full(4, top, np.float32)
            assert sorted(canon_action.tolist()) == [0, 0, 1, 1, 2, 2, 3, 3]
        else:
            row = np.float32(m["reward"].min()) - np.float32(1.0) - np.float32(0.25) * np.arange(4, dtype=np.float32)
            row[ac] = top
            assert (canon_action == ac).all()
        # the lanes' greedy env actions, from the row in each lane's own frame (first maximum)
        assert np.array_equal(np.argmax(ST.env_rows(np.repeat(row[None], 8, axis=0), g), axis=1), env_action)
        next_keys = {(int(k) if k else 1,) for k in ST.canon(m["boards"])[2]}
        _FUSED["sym", pairs] = dict(m=m, row=row, key_s=(int(ckeys[0]),), canon_action=canon_action, next_keys=next_keys)
    return _FUSED["sym", pairs]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("pairs", [False, True])
def test_fused_step_on_the_eight_images_of_one_board(pkg, O, dev, pairs):
    """Q2048_FLAG_SYMMETRIC, 4x4: the eight images are eight different boards and ONE table row.  With one maximum in
    the canonical row the eight lanes meet in one entry -- c_8 in strict mode; with four equal values they meet in pairs
    in four entries, each of which ends as c_2 of its own chain (its pair's reward) without disturbing the other
    three."""
    L, n, words, lr, gamma, cap_log2 = lib(pkg, dev), 4, 1, 0.1, 0.9, 8
    w = symmetric_world(O, pairs)
    m, key_s, ca = w["m"], w["key_s"], w["canon_action"]
    image = M.build_image(cap_log2, np.array([key_s], dtype=U), w["row"][None], 1)
    entries = sorted(set(ca.tolist()))
    K = 8 // len(entries)
    chains = {c: chain_of(w["row"][c], m["reward"][ca == c][0], lr, gamma, K) for c in entries}
    for flags in (0, TD_CAS):
        what, strict = f"symmetric pairs={pairs} flags={flags}", bool(flags & TD_CAS)
        table = new_table(dev, cap_log2, image)
        got = call_fused(L, dev, table, cap_log2, m["before"], m["aux"], n, lr, gamma, SYMMETRIC | flags)
        after = raw(table)
        assert_fused_outputs(got, m, 8, len(w["next_keys"]), strict, what)
        retries, fallbacks = int(got[2][ST_CAS_RETRY]), int(got[2][ST_CAS_FALLBACK])
        check_counters(dev, retries, fallbacks, K, strict, True, what, entries=len(entries))
        d = {key_s: w["row"].copy(), **{k: np.zeros(4, np.float32) for k in w["next_keys"]}}
        for c in entries:
            bits = entry_bits(after, key_s, c, words)
            depth = check_entry(bits, chains[c], K, strict, f"{what} entry {c}")
            observed(dev, f"{what} entry {c}", retries, fallbacks, depth, K)
            d[key_s][c] = np.array([bits], dtype=np.uint32).view(np.float32)[0]
        assert_rows_equal_dict(after, d, n, what)
        M.check_structure(after, words, M.ROLLOUT_PROBE)
        assert_teeth(bits, chains[entries[-1]], K, strict, after, words)
