"""The deterministic step -- k_det_phase1 / k_det_phase1_visits, the two-pass radix partition, k_det_apply and
fold_long_run -- on CROWDS OF UPDATES BUILT BY HAND, through q2048_det_rollout / q2048_det_rollout_cached and ctypes alone.

Boards, aux records, table bytes, row-cache records and the workspace are written by the test; what a call leaves is read
back as bytes.  The model shares no code with the product and has three parts:

  semantics  `O.rollout_sync` on an `O.Agent(storage_f32=True)` -- the sequential agent fed the step's transitions in env
             order, which is the specification (include/q2048.h, "Deterministic mode") -- run one step at a time so that the
             float32 running return of the aux record can be restated (the accumulator is rounded to float32 after every
             step) and, for a closed key set without a row cache, so that the envs' visit rows end with every step.
  table      never empty: every crafted state has a row, and so has every successor (each action, moved, each spawn cell
             and value), so the lanes of one (state, action) group carry DIFFERENT TD targets.  With lr = 0.5 every fold
             order, every update folded twice and every update left out changes bits.  The rows are loaded into the
             oracle agent through its update_q_value, the agent is dumped and the device image is `M.build_image` of the
             dump, written as bytes.
  placement  hash16 = ((M.key_hash(key) >> 48) ^ (action * 0x5555)) & 0xffff per lane, the action from `O.draws`,
             `O.draw_uniform`, `O.draw_action` and the first maximum of the row; a dropped update (closed key set, no row)
             has hash 0.  The sorted array is the stable sort of the lanes by hash16.  Every case asserts from this model,
             before it looks at the device, that the run it is about has the length, the number of distinct groups and the
             position it was built for.

States whose (state, action) hashes collide are found by bucketing 6 000 000 random boards by hash16, once per board
size.  Every comparison is exact -- bytes, integers, float32 bit patterns -- except the reward sum, a sum of doubles in an
order the device does not fix, which is bounded by (number of terms) * 2^-53 * sum |r|.

What cannot be built as the kernel comments might suggest, and what is built instead:
  - two long runs whose heads fall in ONE WAVE: a long run holds more than kDetRun = 64 updates and a wave is 64 sorted
    updates, so two heads are at least 65 apart: k_det_apply's `heads` loop runs at most once per wave.  Case 4 puts two
    crowded long runs back to back with their heads in neighbouring waves of one block, the second across the block's end.
  - a (state, action) group whose lanes differ in `done` by the board alone: the move, and so `valid` and the board the
    game-over test sees, are one for the whole group.  Case 6 gives every other lane of a crowd a consecutive-action
    count of 100 (Game2048_env.py:121-123 ends the episode above 100), so one group folds targets with and without
    bootstrap.
  - an empty row-cache record has key 0 "whatever else it holds" (tests/table_model.py): the two libraries leave different
    bytes behind the key, so an env without a visit row is checked for key 0 and a visit row for all of its bytes."""
import ctypes as C
import gc
import time

import numpy as np
import pytest
import torch

import table_model as M
from table_model import U
from test_four_call_kernels import (CANARY, assert_canary_beyond, aux_of, bits, cache_of, canary, dev_of, host_bytes,
                                    key_tuples, rows_dict, u8, words_of)
from test_table_kernels import DEVICES, lib, new_table, raw

SEED, ID0, LR, GAMMA = 31, 5, 0.5, 0.9
NO_NEW_ROWS, TABLE_FULL, ERR_SIZE = 128, 4, -2
RUN, WAVE, BLOCK, TILE = 64, 64, 256, 2048            # kDetRun, a wave, k_det_apply's block, the sort's tile
LOW = 0x400                                            # fillers hash below this, crafted runs (but the run of hash 0) at or above
ONE_STATE_B = [1, 2, 63, 64, 65, 66, 255, 256, 257, 2047, 2048, 2049, 4097]
f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------
# colliding states
# ---------------------------------------------------------------------------------------------------------------
_BUCKETS = {}
XOR = [a * 0x5555 for a in range(4)]


def top16(cells, n):
    return (M.key_hash(M.state_key(cells, n), words_of(n)) >> U(48)).astype(np.int64)


def buckets(n):
    """6 000 000 random boards of cells 0..11, bucketed by the top 16 bits of their key's hash.  -> dict:
      h      the fullest bucket at or above LOW
      fam    a -> the distinct states of bucket h ^ XOR[a]: such a state with action a has hash16 h
      zero   a -> the distinct states of bucket XOR[a]: such a state with action a has hash16 0
      low    distinct states with 0 < top16 < LOW (fillers: with action 0 they sort before every crafted run)
      spare  distinct states of buckets at or above LOW that no case uses for a crowd (absent states)"""
    if n not in _BUCKETS:
        rng = np.random.default_rng(2048 + n)
        cells, h = [], []
        for _ in range(12):
            c = rng.integers(0, 12, size=(500_000, n * n), dtype=np.uint8)
            cells.append(c)
            h.append(top16(c, n).astype(np.uint16))
        cells, h = np.concatenate(cells), np.concatenate(h)
        counts = np.bincount(h, minlength=1 << 16)
        counts[:LOW] = 0
        top = int(np.argmax(counts))

        def bucket(x):
            return np.unique(cells[h == x], axis=0)

        fam, zero = {a: bucket(top ^ XOR[a]) for a in range(4)}, {a: bucket(XOR[a]) for a in range(4)}
        assert len(fam[0]) >= 130, f"{n}x{n}: the fullest bucket holds {len(fam[0])} states: a broken generator"
        assert all(len(zero[a]) >= 40 for a in range(4))
        low = np.unique(cells[(h > 0) & (h < LOW)][:6000], axis=0)
        low = low[np.random.default_rng(n).permutation(len(low))]
        used = {top ^ x for x in XOR} | set(XOR)
        spare = cells[(h >= LOW) & ~np.isin(h, list(used))][:2000]
        spare = np.unique(spare, axis=0)
        spare = spare[np.random.default_rng(n + 1).permutation(len(spare))]
        assert len(low) >= 4200 and len(spare) >= 1500
        _BUCKETS[n] = dict(h=top, fam=fam, zero=zero, low=low, spare=spare)
    return _BUCKETS[n]


def family_groups(n, count):
    """`count` (state, action) pairs that all have hash16 h, the actions 0, 1, 2, 3 in turn."""
    bk = buckets(n)
    out, taken = [], {a: 0 for a in range(4)}
    while len(out) < count:
        a = len(out) % 4
        if taken[a] >= len(bk["fam"][a]):
            a = 0
        out.append((bk["fam"][a][taken[a]], a))
        taken[a] += 1
    return out


# ---------------------------------------------------------------------------------------------------------------
# the table that is not empty
# ---------------------------------------------------------------------------------------------------------------
def successors(O, board, n):
    """Every board one step can lead to: each action that moves something, each empty cell, a 2 or a 4."""
    out = []
    for a in range(4):
        moved, _, ok = O.move(board, a, n)
        if not ok:
            continue
        empty = np.flatnonzero(moved == 0)
        s = np.repeat(moved[None], 2 * len(empty), axis=0)
        s[np.arange(len(empty)), empty] = 1
        s[len(empty) + np.arange(len(empty)), empty] = 2
        out.append(s)
    return np.concatenate(out) if out else np.zeros((0, n * n), np.uint8)


class World:
    """The rows a case's table holds before the call: boards [R, n * n] and float32 values [R, 4]."""

    def __init__(self, n, seed):
        self.n, self.rng, self.index, self.cells, self.q = n, np.random.default_rng(seed), {}, [], []
        self._image = {}

    def add(self, board, q):
        key = np.asarray(board, np.uint8).tobytes()
        if key in self.index:
            return False
        self.index[key] = len(self.cells)
        self.cells.append(np.asarray(board, np.uint8).copy())
        self.q.append(np.asarray(q, f32))
        return True

    def add_crowd(self, O, pairs, with_successors=True):
        """(state, action) pairs: the state's row has its only maximum at that action; the successors' rows hold one
        positive value each, so their maxima differ."""
        for s, a in pairs:
            q = self.rng.uniform(-4, 4, 4).astype(f32)
            q[a] = f32(5 + self.rng.uniform(0, 2))
            self.add(s, q)
        if with_successors:
            for s, _ in pairs:
                for s2 in successors(O, s, self.n):
                    q = np.zeros(4, f32)
                    q[self.rng.integers(4)] = f32(self.rng.uniform(0.25, 8))
                    self.add(s2, q)

    def add_fillers(self, boards):
        """Singleton states whose greedy action is 0."""
        for s in boards:
            assert self.add(s, [f32(self.rng.uniform(0.5, 2)), 0, 0, 0])

    def agent(self, O, eps):
        """A fresh oracle agent with float32 rows that holds exactly these rows, each entry set through update_q_value:
        with lr = 0.5, Q = 0 + 0.5 * (2 v + gamma * 0 - 0) = v."""
        oa = O.Agent(100, 4, LR, GAMMA, eps, n=self.n, storage_f32=True)
        keys = np.zeros((len(self.cells), O.MAXCELLS), np.uint8)
        keys[:, :self.n * self.n] = np.array(self.cells)
        fn, h, base, P = O.lib().orc_agent_update, oa._h, keys.ctypes.data, C.POINTER(C.c_uint8)
        for r, q in enumerate(np.array(self.q, f64).tolist()):
            p = C.cast(base + O.MAXCELLS * r, P)
            some = False
            for a in range(4):
                if q[a] != 0.0:
                    fn(h, p, a, 2.0 * q[a], p, 1)
                    some = True
            if not some:
                fn(h, p, 0, 0.0, p, 1)
        assert len(oa) == len(self.cells)
        return oa

    def image(self, O, cap_log2):
        """The device image of the agent's dump, and its rows read back from the image's words."""
        if cap_log2 not in self._image:
            keys, vals = self.agent(O, 0.0).dump()
            assert np.array_equal(vals.astype(f32).astype(f64), vals)
            words = words_of(self.n)
            image = M.build_image(cap_log2, M.state_key(keys, self.n), vals.astype(f32), words)
            M.check_structure(image, words, M.ROLLOUT_PROBE)
            d = rows_dict(image, self.n)
            want = dict(zip(key_tuples(M.state_key(np.array(self.cells), self.n), self.n), self.q))
            assert d.keys() == want.keys() and all(np.array_equal(bits(d[k]), bits(want[k])) for k in d)
            self._image[cap_log2] = (image, d)
        return self._image[cap_log2]


def cap_for(rows):
    return max(10, int(2 * rows - 1).bit_length())            # load <= 0.5


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def fresh_envs(O, n, boards, seed=SEED, id0=ID0):
    """Env records of a fresh episode whose boards are the crafted ones."""
    envs = O.envs_init(len(boards), n, seed, id0)
    envs["board"][:] = 0
    envs["board"][:, :n * n] = boards
    return envs


def step0_actions(O, d, boards, n, eps, seed=SEED, id0=ID0, ctr=0):
    """The action of every lane in the call's first step, from the rows `d` read from the image's words."""
    kt = key_tuples(M.state_key(boards, n), n)
    greedy = np.array([int(np.argmax(d[k])) if k in d else 0 for k in kt], dtype=np.int64)
    if eps == 0.0:
        return greedy
    x = np.array([O.draws(seed, id0 + i, ctr) for i in range(len(boards))], dtype=np.uint32)
    explore = np.array([O.draw_uniform(int(v)) < eps for v in x[:, 0]])
    return np.where(explore, [O.draw_action(int(v)) for v in x[:, 1]], greedy)


def layout(boards, acts, n, d, closed):
    """The sorted array of the step: the stable sort of the lanes by hash16 (a dropped update has hash 0).
    -> the runs in sorted order: hash, start, length, distinct live groups, drops, the lanes in sorted order, and the
    lanes of every group."""
    words = words_of(n)
    keys = M.state_key(boards, n)
    kt = key_tuples(keys, n)
    live = np.array([not closed or k in d for k in kt])
    h = (((M.key_hash(keys, words) >> U(48)) ^ (np.asarray(acts).astype(U) * U(0x5555))) & U(0xFFFF)).astype(np.int64)
    h[~live] = 0
    order = np.argsort(h, kind="stable")
    hs = h[order]
    starts = np.flatnonzero(np.concatenate([[True], hs[1:] != hs[:-1]]))
    ends = np.concatenate([starts[1:], [len(hs)]])
    runs = []
    for s, e in zip(starts.tolist(), ends.tolist()):
        lanes = order[s:e]
        groups = {}
        for i in lanes.tolist():
            if live[i]:
                groups.setdefault((kt[i], int(acts[i])), []).append(i)
        runs.append(dict(hash=int(hs[s]), start=s, length=e - s, groups=len(groups), drops=int((~live[lanes]).sum()),
                         lanes=lanes, members=groups))
    return runs


def run_of(runs, hash16):
    hit = [r for r in runs if r["hash"] == hash16]
    assert len(hit) == 1, f"no run of hash {hash16:#x}"
    return hit[0]


def distinct_targets(O, d, envs0, acts, lanes, n, seed=SEED, id0=ID0, ctr=0):
    """The TD targets of these lanes, recomputed: one O.Env step per lane, the successor's row from the image."""
    out = set()
    for i in lanes:
        x = O.draws(seed, id0 + int(i), ctr)
        e = O.Env(n)
        e.rec[0] = envs0[i]
        b2, r, done, _, _ = e.step(int(acts[i]), int(x[2]), int(x[3]))
        k2 = key_tuples(M.state_key(b2[None], n), n)[0]
        best = float(np.max(d[k2])) if k2 in d else 0.0
        out.add(float(f32(r)) + GAMMA * best * (0.0 if done else 1.0))
    return out


def assert_some_group_has_distinct_targets(O, d, envs0, acts, runs, n):
    """What makes fold order and double application visible: a group of at least 3 lanes with at least 3 targets."""
    groups = sorted((g for r in runs for g in r["members"].values() if len(g) >= 3), key=len, reverse=True)
    assert groups, "no group of 3 lanes"
    for g in groups[:4]:
        if len(distinct_targets(O, d, envs0, acts, g[:12], n)) >= 3:
            return
    raise AssertionError("the lanes of every group carry the same targets: the table does not show the fold")


class Expect:
    pass


def run_model(O, world, envs, n, eps, calls, closed=False, visits=True, seed=SEED, id0=ID0):
    """The oracle over `calls` (steps per call), one step at a time.  -> (envs before, [Expect per call]): boards, aux
    records, the agent's rows sorted by key, the integer statistics (inserts = the rows the call created), the reward
    sum and sum |r|, per step the lanes whose episode ended, and the envs' visit rows."""
    cells, words = n * n, words_of(n)
    oa = world.agent(O, eps)
    if closed:
        oa.freeze()
    envs0, B = envs.copy(), len(envs)
    keep = B <= (1 << 17)
    out, ctr = [], 0
    for steps in calls:
        e = Expect()
        e.steps, rows0 = steps, len(oa)
        e.si, e.reward, e.abs_reward, e.ended = np.zeros(O.ST_NI, np.int64), 0.0, 0.0, []
        for _ in range(steps):
            if closed and not visits:
                envs["visit_valid"] = 0                               # no row cache: a visit row ends with its step
            before = envs.copy() if keep else None
            ret0, ep0 = envs["episode_return"].copy(), envs["episode"].copy()
            si, sf = O.rollout_sync(envs, oa, 1, seed, id0, ctr)
            e.si += si
            e.reward += float(sf[O.SF_REWARD])
            same = envs["episode"] == ep0
            delta = envs["episode_return"][same] - ret0[same]        # exact: the sum of two float32 values in double
            assert np.array_equal(delta.astype(f32).astype(f64), delta)
            e.abs_reward += float(np.abs(delta).sum())
            ended = np.flatnonzero(~same)
            assert keep or len(ended) == 0
            for i in ended.tolist():                                  # (a reset keeps consecutive_action: the last action)
                x = O.draws(seed, id0 + i, ctr)
                env = O.Env(n)
                env.rec[0] = before[i]
                _, r, done, _, _ = env.step(int(envs["consecutive_action"][i]), int(x[2]), int(x[3]))
                assert done
                e.abs_reward += abs(float(f32(r)))
            e.ended.append(ended)
            envs["episode_return"] = envs["episode_return"].astype(f32).astype(f64)   # the aux record's float32 accumulator
            ctr += 1
        e.si[O.ST_INSERTS] = len(oa) - rows0
        assert e.si[O.ST_DROPS] == (oa.drops if len(out) == 0 else oa.drops - out[-1].drops_total)
        e.drops_total = oa.drops
        keys, vals = oa.dump()
        assert np.array_equal(vals.astype(f32).astype(f64), vals)
        e.rows = M.sort_rows(M.state_key(keys, n), vals.astype(f32), words)
        e.boards, e.aux = envs["board"][:, :cells].copy(), aux_of(envs)
        e.visit = (envs["visit_key"][:, :cells].copy(), envs["visit_q"].astype(f32), envs["visit_valid"] != 0)
        out.append(e)
    return envs0, out


# ---------------------------------------------------------------------------------------------------------------
# the device (or the twin)
# ---------------------------------------------------------------------------------------------------------------
def workspace(dev, need):
    """`need` bytes at a 256-byte boundary inside a buffer of canary bytes -> (buffer, offset of the workspace)."""
    buf = torch.full((need + 768,), CANARY, dtype=torch.uint8, device=dev)
    return buf, (-buf.data_ptr()) % 256


def assert_rows(after, want, n, what):
    words = words_of(n)
    M.check_structure(after, words, M.ROLLOUT_PROBE)                 # (no key twice, every row reachable)
    keys, q = M.rows_of(after, words)
    wk, wq = want
    assert len(keys) == len(wk), f"{what}: {len(keys)} rows in the bytes, the oracle has {len(wk)}"
    assert np.array_equal(keys, wk), f"{what}: key sets differ"
    bad = bits(q) != bits(wq)
    assert not bad.any(), (f"{what}: {int(bad.sum())} entries of {int(bad.any(axis=1).sum())} rows differ in their bits, "
                           f"first at {np.argwhere(bad)[0]}: {q[bad][0]!r} != {wq[bad][0]!r}")


def assert_records(n, cache, e, tag, what):
    """A visit row of the oracle is a record without a slot under the table's tag, byte for byte; an env without one
    has an empty record: key 0."""
    key, q, valid = e.visit
    B, size = len(valid), M.RECORD[n].itemsize
    now = host_bytes(cache).reshape(-1, size)
    assert (now[B:] == CANARY).all(), f"{what}: records beyond B were written"
    want = M.pack_records(n, M.state_key(key, n), q, M.ROWLESS, tag).view(np.uint8).reshape(B, size)
    bad = np.flatnonzero(valid & (now[:B] != want).any(axis=1))
    assert len(bad) == 0, f"{what}: the visit row of lane {bad[0]}: {now[bad[0]].tolist()} != {want[bad[0]].tolist()}"
    got = now[:B].copy().reshape(-1).view(M.RECORD[n])
    bad = np.flatnonzero(~valid & (got["key"] != 0))
    assert len(bad) == 0, f"{what}: lane {bad[0]} has no visit row, its record is not empty"
    return int(valid.sum())


def run_device(pkg, O, dev, n, image, cap_log2, envs0, expects, eps, flags=0, cached=False, seed=SEED, id0=ID0, what=""):
    """The calls of `expects` on buffers the test wrote, each compared with the model as the module's docstring says."""
    L, cells, B, words = lib(pkg, dev), n * n, len(envs0), words_of(n)
    table = new_table(dev, cap_log2, image)
    tb = torch.cat([u8(dev, envs0["board"][:, :cells]).reshape(-1), canary(dev, 64)])
    ta = torch.cat([dev_of(dev, aux_of(envs0).view(np.uint8).reshape(B, 16), torch.uint8).reshape(-1), canary(dev, 64)])
    need = L.q2048_det_workspace_bytes(B, cap_log2)
    assert need >= 256 and need % 256 == 0
    buf, off = workspace(dev, need)
    cache = cache_of(dev, np.zeros(B, M.RECORD[n]), extra=8) if cached else None
    ctr = 0
    for c, e in enumerate(expects):
        tag = f"{what} call {c}"
        stats0 = np.arange(100, 100 + 32, dtype=np.int64)
        si, sf = torch.from_numpy(stats0.copy()).to(dev), torch.zeros(4, dtype=torch.float64, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        args = (tb.data_ptr(), ta.data_ptr(), table.data_ptr(), cap_log2, B, n, e.steps, eps, LR, GAMMA, seed, id0, ctr,
                flags, si.data_ptr(), sf.data_ptr(), st.data_ptr(), buf.data_ptr() + off, need)
        if cached:
            rc = L.q2048_det_rollout_cached(*args, cache.data_ptr(), None)
        else:
            rc = L.q2048_det_rollout(*args, None)
        assert rc == 0, tag
        ctr += e.steps
        assert int(st.item()) == 0, f"{tag}: status {int(st.item())}"
        got = host_bytes(tb)
        bad = np.flatnonzero((got[:B * cells].reshape(B, cells) != e.boards).any(axis=1))
        assert len(bad) == 0, f"{tag}: boards of {len(bad)} lanes differ, first lane {bad[0]}"
        assert_canary_beyond(tb, B * cells, f"{tag} boards")
        got = host_bytes(ta)[:16 * B].reshape(B, 16)
        bad = np.flatnonzero((got != e.aux.view(np.uint8).reshape(B, 16)).any(axis=1))
        assert len(bad) == 0, f"{tag}: aux of {len(bad)} lanes differ, first lane {bad[0]}: {got[bad[0]].view(e.aux.dtype)} != {e.aux[bad[0]]}"
        assert_canary_beyond(ta, 16 * B, f"{tag} aux")
        assert_rows(raw(table), e.rows, n, tag)
        delta = si.cpu().numpy() - stats0
        assert np.array_equal(delta, e.si), f"{tag}: statistics {delta.tolist()}, the oracle has {e.si.tolist()}"
        assert e.si[O.ST_STEPS] == B * e.steps
        f = sf.cpu().numpy()
        bound = B * e.steps * 2.0 ** -53 * e.abs_reward
        print(f"{tag}: reward sum {f[O.SF_REWARD]!r}, the oracle's {e.reward!r}, bound {bound:.3e}")
        assert abs(f[O.SF_REWARD] - e.reward) <= bound, f"{tag}: reward sum off by {abs(f[O.SF_REWARD] - e.reward):.3e} > {bound:.3e}"
        assert f[3] == 0.0
        assert (host_bytes(buf[:off]) == CANARY).all() and (host_bytes(buf[off + need:]) == CANARY).all(), \
            f"{tag}: written outside the workspace's {need} bytes"
        if cached:
            assert_records(n, cache, e, M.cache_tag(table.data_ptr(), cap_log2), tag)
    assert pkg._native.claim_timeouts(L) == 0
    return table


_MODELS = {}


def shared(key, make):
    """A case's model is computed once and shared by the two devices."""
    if key not in _MODELS:
        _MODELS[key] = make()
    return _MODELS[key]


def shuffled(count, seed):
    return np.random.default_rng(seed).permutation(count)


# ---------------------------------------------------------------------------------------------------------------
# 1. one state, one group
# ---------------------------------------------------------------------------------------------------------------
def one_state(O, n):
    """A state of the fullest bucket and an action that moves it and leaves two empty cells or more."""
    for s in buckets(n)["fam"][0]:
        for a in range(4):
            moved, _, ok = O.move(s, a, n)
            if ok and int((moved == 0).sum()) >= 2:
                return s, a
    raise AssertionError("no such state")


def one_state_model(O, n):
    def make():
        s, a = one_state(O, n)
        world = World(n, 10 + n)
        world.add_crowd(O, [(s, a)])
        cap_log2 = cap_for(len(world.cells) + 2 * 3 * max(ONE_STATE_B))
        image, d = world.image(O, cap_log2)
        cases = {}
        for B in ONE_STATE_B:
            boards = np.repeat(s[None], B, axis=0)
            acts = step0_actions(O, d, boards, n, 0.0)
            runs = layout(boards, acts, n, d, False)
            assert (acts == a).all() and len(runs) == 1
            assert runs[0]["start"] == 0 and runs[0]["length"] == B and runs[0]["groups"] == 1
            for calls in ((3,), (1, 2)):
                envs0, ex = run_model(O, world, fresh_envs(O, n, boards), n, 0.0, calls)
                cases[B, calls] = (envs0, ex)
            if B >= 3:
                assert_some_group_has_distinct_targets(O, d, envs0, acts, runs, n)
        assert all(np.array_equal(bits(cases[B, (3,)][1][-1].rows[1]), bits(cases[B, (1, 2)][1][-1].rows[1])) for B in ONE_STATE_B)
        return world, cap_log2, image, cases
    return shared(("one", n), make)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_one_state_one_group(pkg, O, dev, n):
    """Case 1.  Every lane on one board whose row has one maximum, eps = 0: one run of B updates, one group.  B = 1 and 2,
    the short path up to 64, the long path from 65, a run across a wave, a block, one and two sort tiles.  3 steps in one
    call, and 1 + 2 steps with the counter carried (the held slot crosses steps, not calls)."""
    world, cap_log2, image, cases = one_state_model(O, n)
    for B in ONE_STATE_B:
        for calls in ((3,), (1, 2)):
            envs0, ex = cases[B, calls]
            run_device(pkg, O, dev, n, image, cap_log2, envs0, ex, 0.0, what=f"B={B} steps={calls}")


# ---------------------------------------------------------------------------------------------------------------
# 2. the short/long boundary with mixed groups, at chosen sorted indices
# ---------------------------------------------------------------------------------------------------------------
LENGTHS, GROUPS = [63, 64, 65, 66, 129], [2, 3, 64]
STARTS = [63, 64, 255, 256, 257, 2047, 2048]


def crowd_batch(bk, pairs, sizes, fillers, seed):
    """Boards of a batch: group j (a (state, action) pair) on sizes[j] lanes, `fillers` singleton lanes, all in one
    fixed shuffle of env order."""
    boards = [pairs[j][0] for j, k in enumerate(sizes) for _ in range(k)] + list(bk["low"][:fillers])
    boards = np.array(boards, dtype=np.uint8)
    return boards[shuffled(len(boards), seed)]


def boundary_model(O, n, start):
    def make():
        bk = buckets(n)
        pairs = family_groups(n, max(GROUPS))
        world = World(n, 20 + n)
        world.add_crowd(O, pairs)
        world.add_fillers(bk["low"][:start])
        cap_log2 = cap_for(len(world.cells) + 2 * 2 * (start + max(LENGTHS)))
        image, d = world.image(O, cap_log2)
        cases = {}
        for length in LENGTHS:
            for g in GROUPS:
                g = min(g, length)                                    # (63 updates hold 63 groups at the most)
                sizes = np.bincount(np.arange(length) % g, minlength=g)
                boards = crowd_batch(bk, pairs, sizes, start, 1000 * length + g)
                acts = step0_actions(O, d, boards, n, 0.0)
                runs = layout(boards, acts, n, d, False)
                run = run_of(runs, bk["h"])
                assert (run["start"], run["length"], run["groups"]) == (start, length, g)
                assert all(r["hash"] < LOW for r in runs if r is not run)
                inside = [bool(np.all(np.diff(m) > 0)) for m in run["members"].values()]
                assert all(inside), "the stable sort keeps a group's lanes in env order"
                if g <= 3:                                            # interleaved, not in blocks: every group begins
                    first = [m[0] for m in run["members"].values()]   # before any group ends
                    last = [m[-1] for m in run["members"].values()]
                    assert max(first) < min(last)
                envs0, ex = run_model(O, world, fresh_envs(O, n, boards), n, 0.0, (2,))
                if g <= 3:
                    assert_some_group_has_distinct_targets(O, d, envs0, acts, [run], n)
                cases[length, g] = (envs0, ex)
        return cap_log2, image, cases
    return shared(("boundary", n, start), make)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("start", STARTS)
@pytest.mark.parametrize("n", [4, 5])
def test_short_long_boundary_with_mixed_groups(pkg, O, dev, n, start):
    """Case 2.  One run of 63, 64, 65, 66 and 129 updates (long above 64), made of 2, 3 and 64 groups interleaved in env
    order, that begins at sorted index `start`: the last lane of a wave and the first of the next, either side of a
    block's end, either side of a sort tile's end.  The index is reached with filler lanes on singleton states of
    smaller hash16; two steps."""
    cap_log2, image, cases = boundary_model(O, n, start)
    for (length, g), (envs0, ex) in cases.items():
        run_device(pkg, O, dev, n, image, cap_log2, envs0, ex, 0.0, what=f"start={start} length={length} groups={g}")


# ---------------------------------------------------------------------------------------------------------------
# 3. more than 64 groups in a long run
# ---------------------------------------------------------------------------------------------------------------
def many_groups_model(O, n, groups):
    def make():
        bk, fillers = buckets(n), 37
        pairs = family_groups(n, groups)
        world = World(n, 30 + n)
        world.add_crowd(O, pairs)
        world.add_fillers(bk["low"][:fillers])
        sizes = np.ones(groups, np.int64) if groups == RUN else 1 + (np.arange(groups) * 5 + 2) % 8
        boards = crowd_batch(bk, pairs, sizes, fillers, 300 + groups)
        cap_log2 = cap_for(len(world.cells) + 2 * 2 * len(boards))
        image, d = world.image(O, cap_log2)
        acts = step0_actions(O, d, boards, n, 0.0)
        runs = layout(boards, acts, n, d, False)
        run = run_of(runs, bk["h"])
        assert (run["start"], run["length"], run["groups"]) == (fillers, int(sizes.sum()), groups)
        if groups == RUN:
            assert run["length"] == RUN                               # the short path, every update a group's head
        else:
            assert run["length"] > RUN and -(-groups // 64) == {65: 2, 128: 2, 129: 3, 130: 3}[groups]
            assert sorted(len(m) for m in run["members"].values()) == sorted(sizes.tolist()) and sizes.max() == 8
            order = [min(m) for m in run["members"].values()]        # groups in order of first appearance: who owns a
            late = np.argsort(order)[64:]                             # lane in the first sweep, who waits for a later one
            assert len(late) == groups - 64
            assert_some_group_has_distinct_targets(O, d, fresh_envs(O, n, boards), acts, [run], n)
        envs0, ex = run_model(O, world, fresh_envs(O, n, boards), n, 0.0, (2,))
        return cap_log2, image, envs0, ex
    return shared(("many", n, groups), make)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("groups", [64, 65, 128, 129, 130])
@pytest.mark.parametrize("n", [4, 5])
def test_more_than_64_groups_in_a_long_run(pkg, O, dev, n, groups):
    """Case 3, on the library that ships.  One long run of 65, 128, 129 and 130 distinct groups of 1 to 8 lanes, shuffled:
    fold_long_run owns 64 groups per sweep, so it takes 2, 2, 3 and 3 sweeps.  And one run of 64 updates that are 64
    groups: the short path with every update the head of its group."""
    cap_log2, image, envs0, ex = many_groups_model(O, n, groups)
    run_device(pkg, O, dev, n, image, cap_log2, envs0, ex, 0.0, what=f"groups={groups}")


# ---------------------------------------------------------------------------------------------------------------
# 4. two crowded long runs in one block; a long run whose head is a block's last lane
# ---------------------------------------------------------------------------------------------------------------
def two_runs_model(O, n, fillers, len_a, len_b):
    def make():
        bk = buckets(n)
        h = bk["h"]
        other = max((a for a in (1, 2, 3) if (h ^ XOR[a]) >= LOW), key=lambda a: len(bk["fam"][a]))
        h2 = h ^ XOR[other]
        # run `h`: 9 groups of the family (actions 0..3); run `h2`: 7 states of bucket h2 with action 0
        pairs_a = family_groups(n, 9)
        pairs_b = [(s, 0) for s in bk["fam"][other][40:47]]
        assert not {s.tobytes() for s, _ in pairs_a} & {s.tobytes() for s, _ in pairs_b}
        first, second = (pairs_a, pairs_b) if h < h2 else (pairs_b, pairs_a)
        world = World(n, 40 + n)
        world.add_crowd(O, pairs_a + pairs_b)
        world.add_fillers(bk["low"][:fillers])
        sizes = np.concatenate([np.bincount(np.arange(len_a) % len(first), minlength=len(first)),
                                np.bincount(np.arange(len_b) % len(second), minlength=len(second))])
        boards = crowd_batch(bk, first + second, sizes, fillers, 400 + fillers)
        cap_log2 = cap_for(len(world.cells) + 2 * 2 * len(boards))
        image, d = world.image(O, cap_log2)
        acts = step0_actions(O, d, boards, n, 0.0)
        runs = layout(boards, acts, n, d, False)
        ra, rb = run_of(runs, min(h, h2)), run_of(runs, max(h, h2))
        assert (ra["start"], ra["length"], ra["groups"]) == (fillers, len_a, len(first))
        assert (rb["start"], rb["length"], rb["groups"]) == (fillers + len_a, len_b, len(second))
        assert ra["length"] > RUN and rb["length"] > RUN
        assert_some_group_has_distinct_targets(O, d, fresh_envs(O, n, boards), acts, [ra, rb], n)
        envs0, ex = run_model(O, world, fresh_envs(O, n, boards), n, 0.0, (2,))
        return cap_log2, image, envs0, ex, (ra["start"], rb["start"], rb["start"] + rb["length"])
    return shared(("two", n, fillers, len_a, len_b), make)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_two_crowded_long_runs_in_one_block(pkg, O, dev, n):
    """Case 4.  Two long runs of several groups back to back: the heads at sorted index 130 and 195 -- neighbouring waves
    of the first block (two heads in one wave cannot be: see the module's docstring) -- the second run across the
    block's end.  Then a crowded long run whose head is lane 63 of the last wave of a block (sorted index 255), followed
    by a second one."""
    cap_log2, image, envs0, ex, (a, b, end) = two_runs_model(O, n, 130, 65, 100)
    assert a // BLOCK == b // BLOCK and b // WAVE == a // WAVE + 1 and end > BLOCK
    run_device(pkg, O, dev, n, image, cap_log2, envs0, ex, 0.0, what="heads at 130 and 195")
    cap_log2, image, envs0, ex, (a, b, end) = two_runs_model(O, n, 255, 70, 66)
    assert a % BLOCK == BLOCK - 1 and a % WAVE == WAVE - 1
    run_device(pkg, O, dev, n, image, cap_log2, envs0, ex, 0.0, what="head at 255")


# ---------------------------------------------------------------------------------------------------------------
# 5. closed key set: dropped updates next to live groups
# ---------------------------------------------------------------------------------------------------------------
def stuck_board(O, n):
    """A board on which neither action 0 nor action 1 moves anything and another action does: full rows, full columns
    or a full first row and column (in its four orientations), no two equal neighbours."""
    i = np.arange(n * n)
    full = (1 + (i // n + i % n) % 2 + 2 * (i % 3 == 0)).astype(np.uint8).reshape(n, n)
    rows = np.where((np.arange(n) % 2 == 0)[:, None], full, 0)
    corner = np.where((np.arange(n)[:, None] == 0) | (np.arange(n)[None, :] == 0), full, 0)
    for b in [rows, rows.T] + [np.rot90(corner, k) for k in range(4)]:
        b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
        if not O.move(b, 0, n)[2] and not O.move(b, 1, n)[2] and (O.move(b, 2, n)[2] or O.move(b, 3, n)[2]):
            return b
    raise AssertionError("no such board")


def closed_model(O, n, absent_lanes, cached):
    def make():
        bk = buckets(n)
        live = [(s, a) for a in range(4) for s in bk["zero"][a][:3]]          # 12 groups of hash16 0
        world = World(n, 50 + n)
        world.add_crowd(O, live)
        elsewhere = 20
        world.add_fillers(bk["low"][:elsewhere])
        stuck = stuck_board(O, n)
        stay = min(5, absent_lanes // 2)
        gone = [stuck] * stay + list(bk["spare"][:absent_lanes - stay])
        assert all(np.asarray(s, np.uint8).tobytes() not in world.index for s in gone)
        sizes = 2 + np.arange(len(live)) % 4
        boards = [live[j][0] for j, k in enumerate(sizes) for _ in range(k)] + list(bk["low"][:elsewhere]) + gone
        boards = np.array(boards, dtype=np.uint8)
        boards = boards[shuffled(len(boards), 500 + absent_lanes)]
        cap_log2 = cap_for(len(world.cells))
        image, d = world.image(O, cap_log2)
        acts = step0_actions(O, d, boards, n, 0.0)
        runs = layout(boards, acts, n, d, True)
        run = run_of(runs, 0)
        assert run["start"] == 0 and run["drops"] == absent_lanes and run["groups"] == len(live)
        assert run["length"] == absent_lanes + int(sizes.sum())
        dropped = np.array([k not in d for k in key_tuples(M.state_key(boards[run["lanes"]], n), n)])
        assert dropped[1:-1].any() and (~dropped)[1:-1].any() and np.abs(np.diff(dropped.astype(int))).sum() >= 6, \
            "drops and live updates alternate inside the run"
        assert_some_group_has_distinct_targets(O, d, fresh_envs(O, n, boards), acts, [run], n)
        envs0, ex = run_model(O, world, fresh_envs(O, n, boards), n, 0.0, (2, 2), closed=True, visits=cached)
        on_stuck = np.flatnonzero((boards == stuck).all(axis=1))
        assert len(on_stuck) == stay >= 2
        if cached:                                                    # s' = s: the visit row learned, and crossed the call boundary
            key, q, valid = ex[0].visit
            assert valid[on_stuck].all() and (key[on_stuck] == stuck).all() and (q[on_stuck] != 0).any(axis=1).all()
        assert ex[0].si[O.ST_DROPS] >= absent_lanes and ex[0].si[O.ST_INSERTS] == 0 and ex[1].si[O.ST_INSERTS] == 0
        return cap_log2, image, envs0, ex
    return shared(("closed", n, absent_lanes, cached), make)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("cached", [False, True], ids=["no cache", "row cache"])
@pytest.mark.parametrize("absent_lanes", [10, 64, 65, 300])
@pytest.mark.parametrize("n", [4, 5])
def test_dropped_updates_next_to_live_groups(pkg, O, dev, n, absent_lanes, cached):
    """Case 5.  Q2048_FLAG_NO_NEW_ROWS: 10, 64, 65 and 300 lanes on states without a row -- their updates are dropped
    words of hash 0 -- shuffled among 12 live groups whose hash16 is 0 as well: one run, short or long, that holds both.
    Drops are the oracle's, Q2048_STATUS_TABLE_FULL is not raised, no row is created.  Several lanes sit on a board
    without a row on which action 0 moves nothing: with the row cache their visit row learns in phase 1 and is read in
    the next step and, 2 + 2 steps, in the next call; the records are compared after each call."""
    cap_log2, image, envs0, ex = closed_model(O, n, absent_lanes, cached)
    table = run_device(pkg, O, dev, n, image, cap_log2, envs0, ex, 0.0, flags=NO_NEW_ROWS, cached=cached,
                       what=f"absent={absent_lanes} cached={cached}")
    assert np.array_equal(raw(table)[:, [0, 3]], image[:, [0, 3]]), "the key set changed"


# ---------------------------------------------------------------------------------------------------------------
# 6. episodes end inside a group
# ---------------------------------------------------------------------------------------------------------------
def dead_board(n):
    """A full board without two equal neighbours."""
    i = np.arange(n * n)
    return (1 + ((i // n + i % n) % 2) + 2 * (i % 3 == 0)).astype(np.uint8)


def endings_model(O, n):
    def make():
        bk = buckets(n)
        dead = dead_board(n)
        assert O.is_game_over(dead, n)
        crowd, best = bk["fam"][1][5], 1
        assert O.move(crowd, best, n)[2]
        world = World(n, 60 + n)
        world.add_crowd(O, [(crowd, best), (dead, 2)])
        world.add_fillers(bk["low"][:30])
        boards = np.array([crowd] * 80 + [dead] * 40 + list(bk["low"][:30]), dtype=np.uint8)
        perm = shuffled(len(boards), 600)
        boards = boards[perm]
        envs = fresh_envs(O, n, boards)
        on_crowd = np.flatnonzero((boards == crowd).all(axis=1))
        tired = on_crowd[::2]              # 100 steps of action `best` behind them: the next one ends the episode
        envs["consecutive_action"][tired], envs["consecutive_count"][tired] = best, 100
        envs["last_consecutive_penalty"][tired] = -10.0
        cap_log2 = cap_for(len(world.cells) + 2 * 3 * len(boards))
        image, d = world.image(O, cap_log2)
        acts = step0_actions(O, d, boards, n, 0.5)
        runs = layout(boards, acts, n, d, False)
        group = [m for r in runs for (k, a), m in r["members"].items() if a == best and m[0] in set(on_crowd.tolist())][0]
        envs0, ex = run_model(O, world, envs, n, 0.5, (3,))
        ended = set(ex[0].ended[0].tolist())
        n_end = sum(1 for i in group if i in ended)
        assert len(group) >= 20 and 3 <= n_end <= len(group) - 3, "one group holds lanes that end the episode and lanes that do not"
        assert {i for i in group if i in ended} == set(group) & set(tired.tolist())
        on_dead = np.flatnonzero((boards == dead).all(axis=1))
        assert set(on_dead.tolist()) <= ended and len({int(acts[i]) for i in on_dead}) == 4
        assert ex[0].si[O.ST_EPISODES] >= len(on_dead) + n_end and ex[0].si[O.ST_INSERTS] > 0
        return cap_log2, image, envs0, ex
    return shared(("endings", n), make)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_episodes_end_inside_a_group(pkg, O, dev, n):
    """Case 6, eps = 0.5, 3 steps.  A crowd on one board of which every other lane has repeated the row's best action 100
    times: in the group of that action those lanes end the episode (a target without bootstrap, no held slot, the new
    episode's first state probed in the next step) and the others do not.  A second crowd sits on a dead board: every
    action ends the episode there."""
    cap_log2, image, envs0, ex = endings_model(O, n)
    run_device(pkg, O, dev, n, image, cap_log2, envs0, ex, 0.5, what="endings")


# ---------------------------------------------------------------------------------------------------------------
# 7. the partition's geometry
# ---------------------------------------------------------------------------------------------------------------
GEOMETRY = {4095: (2, 2), 4097: (3, 2), 8193: (5, 4), 34817: (18, 8)}         # B -> (tiles, tiles per group)
SCAN_B = 4096 * TILE + 1                    # the smallest batch beyond 4096 tiles: the partition with its scan launch


def geometry_of(B):
    tiles = -(-B // TILE)
    gsz = 1
    while gsz * gsz < tiles:
        gsz *= 2
    return tiles, gsz


def crowd_world(O, n):
    """64 states, 16 of each bucket of the family: with the four actions, 256 groups in the four runs h ^ XOR[a]."""
    def make():
        bk = buckets(n)
        states = [s for a in range(4) for s in [s for s in bk["fam"][a] if not O.is_game_over(s, n)][50:66]]
        assert len(states) == 64
        world = World(n, 70 + n)
        world.add_crowd(O, [(s, int(j % 4)) for j, s in enumerate(states)])
        return world, np.array(states, dtype=np.uint8)
    return shared(("crowds", n), make)


def geometry_model(O, n, B):
    def make():
        bk = buckets(n)
        world, states = crowd_world(O, n)
        boards = states[np.random.default_rng(B).integers(0, len(states), B)]
        cap_log2 = cap_for(len(world.cells) + 2 * 2 * B)
        image, d = world.image(O, cap_log2)
        tiles, gsz = geometry_of(B)
        assert (tiles, gsz) == GEOMETRY[B] and (tiles % gsz != 0) == (B != 4095), "a partial last group, but for two tiles"
        acts = step0_actions(O, d, boards, n, 0.5)
        runs = layout(boards, acts, n, d, False)
        assert [r["hash"] for r in runs] == sorted(bk["h"] ^ x for x in XOR)
        assert all(r["groups"] == 64 and r["length"] > B // 5 for r in runs)
        assert any(r["start"] // TILE != (r["start"] + r["length"] - 1) // TILE for r in runs)
        assert_some_group_has_distinct_targets(O, d, fresh_envs(O, n, boards), acts, runs, n)
        envs0, ex = run_model(O, world, fresh_envs(O, n, boards), n, 0.5, (2,))
        return cap_log2, image, envs0, ex
    return shared(("geometry", n, B), make)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", list(GEOMETRY))
@pytest.mark.parametrize("n", [4, 5])
def test_partition_geometry(pkg, O, dev, n, B):
    """Case 7.  Random crowds on 64 states x 4 actions, eps = 0.5: four long runs of 64 groups each across the tiles.
    B = 4095, 4097, 8193 and 34 817 are 2, 3, 5 and 18 tiles in groups of 2, 2, 4 and 8 with a partial last group (the
    group sums of k_sort_count / k_sort_scatter); two steps, the table bit exact."""
    cap_log2, image, envs0, ex = geometry_model(O, n, B)
    run_device(pkg, O, dev, n, image, cap_log2, envs0, ex, 0.5, what=f"B={B}")


@pytest.mark.gpu
def test_partition_with_its_scan_launch(pkg, O):
    """Case 7, the one case that cannot be smaller: B = 4096 * 2048 + 1 is the smallest batch at which the library that
    ships launches k_sort_scan (more than 4096 tiles).  4x4, one step, a 2^20-slot table, the crowds of the other
    geometry cases: about 0.6 GB of device memory and one oracle pass over 8 Mi envs."""
    t0 = time.time()
    n, B, cap_log2 = 4, SCAN_B, 20
    assert geometry_of(B)[0] == 4097 and geometry_of(B - 1)[0] == 4096
    world, states = crowd_world(O, n)
    image, d = world.image(O, cap_log2)
    boards = states[np.random.default_rng(B).integers(0, len(states), B)]
    envs0, ex = run_model(O, world, fresh_envs(O, n, boards), n, 0.5, (1,))
    assert ex[0].si[O.ST_EPISODES] == 0 and 0.4 * B < ex[0].si[O.ST_EXPLORE] < 0.6 * B
    t1 = time.time()
    run_device(pkg, O, "cuda:0", n, image, cap_log2, envs0, ex, 0.5, what=f"B={B}")
    print(f"B={B}: the oracle {t1 - t0:.1f} s, the device and the comparison {time.time() - t1:.1f} s")
    del envs0, ex, boards
    gc.collect()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------
# 8. the workspace
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_workspace_size_and_one_byte_less(pkg, O, dev, n):
    """q2048_det_workspace_bytes at every B of case 1: a multiple of 256 that does not shrink as B grows; on the device
    at least the two double-buffered (update word, target) pairs and the held slot of every env -- 36 bytes per env --
    and the per-tile digit counts.  (That the call stays inside it is asserted by every case of this file: a canary
    lies behind it.)  A call with one byte less is refused with Q2048_ERR_SIZE by both libraries and leaves boards, aux,
    table, statistics, status and workspace as they were."""
    L, cells = lib(pkg, dev), n * n
    world, cap_log2, image, cases = one_state_model(O, n)
    sizes = [L.q2048_det_workspace_bytes(B, cap_log2) for B in ONE_STATE_B]
    assert all(s >= 256 and s % 256 == 0 for s in sizes) and sizes == sorted(sizes)
    if dev != "cpu":
        for B, s in zip(ONE_STATE_B, sizes):
            floor = 2 * 2 * 256 * -(-8 * B // 256) + 256 * -(-4 * B // 256) + 4 * 256 * -(-B // TILE)
            assert floor <= s <= floor + (1 << 16), f"B={B}: {s} bytes"
    for B, need in zip(ONE_STATE_B, sizes):
        envs0, _ = cases[B, (3,)]
        table = new_table(dev, cap_log2, image)
        tb, ta = u8(dev, envs0["board"][:, :cells]), dev_of(dev, aux_of(envs0).view(np.uint8).reshape(B, 16), torch.uint8)
        buf, off = workspace(dev, need)
        stats0 = np.arange(100, 132, dtype=np.int64)
        si, sf = torch.from_numpy(stats0.copy()).to(dev), torch.full((4,), 0.5, dtype=torch.float64, device=dev)
        st = torch.zeros(1, dtype=torch.int32, device=dev)
        cache = cache_of(dev, np.zeros(B, M.RECORD[n]))
        args = (tb.data_ptr(), ta.data_ptr(), table.data_ptr(), cap_log2, B, n, 3, 0.0, LR, GAMMA, SEED, ID0, 0)
        rest = (si.data_ptr(), sf.data_ptr(), st.data_ptr(), buf.data_ptr() + off, need - 1)
        assert L.q2048_det_rollout(*args, 0, *rest, None) == ERR_SIZE, f"B={B}"
        assert L.q2048_det_rollout_cached(*args, NO_NEW_ROWS, *rest, cache.data_ptr(), None) == ERR_SIZE, f"B={B}"
        assert np.array_equal(host_bytes(tb).reshape(B, cells), envs0["board"][:, :cells]), f"B={B}: boards"
        assert np.array_equal(host_bytes(ta).reshape(-1), aux_of(envs0).view(np.uint8).reshape(-1)), f"B={B}: aux"
        assert np.array_equal(raw(table), image), f"B={B}: table"
        assert np.array_equal(si.cpu().numpy(), stats0) and (sf.cpu().numpy() == 0.5).all() and int(st.item()) == 0
        assert (host_bytes(buf) == CANARY).all() and not host_bytes(cache).any(), f"B={B}: workspace or row cache"
