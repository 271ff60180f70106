"""Merging Q-tables on the device: q2048_table_merge, BatchedQLearningAgent.merge_from, merge_tables.py.

The checking model is plain numpy on `export_rows()`: the rows of the destination before the call and of the source,
keyed by state, combined by the mode's formula in float32 (every product and sum a numpy operation of its own, so
nothing is fused), compared with the destination's rows afterwards -- same key set, values equal AS BIT PATTERNS.  No
tolerance anywhere.  Every test runs on the CPU twin ("cpu") and on the GPU."""
import ctypes as C
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
ADD, BLEND, MAXABS = 0, 1, 2
MODES = [("add", 1.0), ("add", 0.25), ("blend", 0.0), ("blend", 1.0), ("blend", 0.3), ("maxabs", 1.0)]


def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
def keys2d(keys):
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    return k.reshape(len(k), -1) if k.size else np.zeros((0, 1), np.uint64)


def unique_rows(k):
    """np.unique(k, axis=0, return_index=True, return_inverse=True) for uint64 [R, words], by one lexsort."""
    order = np.lexsort(k.T[::-1])                        # (the first word is the primary key; stable)
    ks = k[order]
    new = np.ones(len(k), bool)
    new[1:] = (ks[1:] != ks[:-1]).any(axis=1)
    inv = np.empty(len(k), np.int64)
    inv[order] = np.cumsum(new) - 1
    return ks[new], order[new], inv


def sorted_rows(keys, q):
    """(keys [R, words], q [R, 4]) sorted by key; asserts that no key occurs twice."""
    k = keys2d(keys)
    if len(k) == 0:
        return k, np.zeros((0, 4), np.float32)
    u, idx, _ = unique_rows(k)
    assert len(u) == len(k), "a key occurs twice in the export"
    return u, np.ascontiguousarray(q, dtype=np.float32)[idx]


def model_merge(dst, src, mode, w):
    """dst, src: (keys, q) as export_rows() gives them.  Returns the merged (keys, q), sorted by key, and how many src
    rows were created / combined.  float32 throughout; 1 - w is computed once in float32, like the host side."""
    dk, dq = sorted_rows(*dst)
    sk, sq = sorted_rows(*src)
    words = max(dk.shape[1] if len(dk) else 0, sk.shape[1] if len(sk) else 0, 1)
    allk = np.concatenate([dk.reshape(-1, words), sk.reshape(-1, words)])
    if len(allk) == 0:
        return allk, np.zeros((0, 4), np.float32), 0, 0
    u, _, inv = unique_rows(allk)
    D, S = np.zeros((len(u), 4), np.float32), np.zeros((len(u), 4), np.float32)
    has_d, has_s = np.zeros(len(u), bool), np.zeros(len(u), bool)
    D[inv[:len(dk)]], has_d[inv[:len(dk)]] = dq, True
    S[inv[len(dk):]], has_s[inv[len(dk):]] = sq, True
    w32 = np.float32(w)
    keep = np.float32(1.0) - w32
    with np.errstate(all="ignore"):
        if mode == "add":
            ws = w32 * S
            both, only_s = D + ws, ws
        elif mode == "blend":
            both, only_s = keep * D + w32 * S, S
        else:
            both, only_s = np.where(np.abs(S) > np.abs(D), S, D), S
    assert both.dtype == np.float32 and only_s.dtype == np.float32
    out = np.where((has_d & has_s)[:, None], both, np.where(has_s[:, None], only_s, D))
    return u, out.astype(np.float32), int((has_s & ~has_d).sum()), int((has_s & has_d).sum())


def locate(sorted_keys, keys):
    """Where each row of `keys` lies in `sorted_keys` (unique, sorted, a superset)."""
    u, _, inv = unique_rows(np.concatenate([sorted_keys, keys.reshape(-1, sorted_keys.shape[1])]))
    assert len(u) == len(sorted_keys), "a key is missing"
    return inv[len(sorted_keys):]


def rows_of(agent):
    """The occupied slots' key and values, sorted: what a run left in its table, wherever the rows lie."""
    t = agent.table.view(torch.int64).reshape(-1, 4)
    return torch.unique(t[t[:, 0] != 0][:, :3], dim=0)


def assert_rows_equal(got, want_keys, want_q, what=""):
    gk, gq = sorted_rows(*got)
    assert gk.shape[0] == want_keys.shape[0], f"{what}: {gk.shape[0]} rows, the model has {want_keys.shape[0]}"
    assert np.array_equal(gk.reshape(want_keys.shape), want_keys), f"{what}: key sets differ"
    bad = gq.view(np.uint32) != np.ascontiguousarray(want_q).view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.any(axis=1).sum())} rows differ in their bits, first at {np.argwhere(bad)[0]}"


# ---------------------------------------------------------------------------------------------
# agents: trained once per (device, board size, seed), copied per case
# ---------------------------------------------------------------------------------------------
_TRAINED = {}


def new_agent(pkg, dev, n, cap, seed=1, **kw):
    kw.setdefault("freeze_load", None)
    return pkg.BatchedQLearningAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.3, capacity_log2=cap,
                                     seed=seed, env_id0=0, device=dev, board_size=n, **kw)


def trained_rows(pkg, dev, n, seed, B=4096, steps=200):
    """The rows of a shared-table learner after `steps` fused steps of B envs on `seed`: (keys, q) on the host."""
    key = (dev, n, seed, B, steps)
    if key not in _TRAINED:
        env = pkg.BatchedGame2048Env(B, board_size=n, seed=seed, env_id0=0, device=dev)
        agent = new_agent(pkg, dev, n, 21, seed=seed)
        for _ in range(steps // 50):
            agent.fused_rollout(env, 50)
        sync(dev)
        assert agent.check_status() == 0 and agent.stats()["drops"] == 0
        agent.verify_table()
        _TRAINED[key] = agent.export_rows()
    return _TRAINED[key]


def agent_with(pkg, dev, n, rows, cap, **kw):
    """A fresh agent whose table holds `rows` = (keys, q)."""
    agent = new_agent(pkg, dev, n, cap, **kw)
    agent.import_rows(*rows)
    return agent


def check_merge(pkg, dst, src, mode, w, what=""):
    """merge_from against the model, with every identity the counters and the bookkeeping owe."""
    before, other = dst.export_rows(), src.export_rows()
    size_before, size_other = dst.table_size(), src.table_size()
    src_table = src.table.clone()
    out = dst.merge_from(src, mode=mode, weight=w)
    sync(dst.device.type)
    mk, mq, created, combined = model_merge(before, other, mode, w)
    assert out["dropped"] == 0 and out["created"] == created and out["combined"] == combined, (what, out, created, combined)
    assert out["read"] == out["created"] + out["combined"] + out["dropped"] == size_other
    assert dst.table_size() == size_before + out["created"]
    dst.verify_table()
    assert pkg._native.claim_timeouts(dst._L) == 0
    assert torch.equal(src.table, src_table), "the source was written"
    assert_rows_equal(dst.export_rows(), mk, mq, what)
    return out, before, other


# ---------------------------------------------------------------------------------------------
# 1. ABI
# ---------------------------------------------------------------------------------------------
def test_both_libraries_export_the_merge(pkg):
    N = pkg._native
    assert "q2048_table_merge" in N._SIGNATURES
    assert (N.MERGE_ADD, N.MERGE_BLEND, N.MERGE_MAXABS) == (ADD, BLEND, MAXABS)
    assert hasattr(C.CDLL(N.HOST_LIB_PATH), "q2048_table_merge")
    assert hasattr(C.CDLL(N.LIB_PATH), "q2048_table_merge")          # loads without a GPU: no compute call here
    assert N.host_lib().q2048_abi_version() == N.lib().q2048_abi_version() == 7   # additive: detected by its symbol
    with open(os.path.join(REPO, "include", "q2048.h")) as fh:
        hdr = fh.read()
    for name, value in (("Q2048_MERGE_ADD", 0), ("Q2048_MERGE_BLEND", 1), ("Q2048_MERGE_MAXABS", 2)):
        assert f"#define {name} {value}" in hdr


@pytest.mark.parametrize("which", ["hip", "host"])
def test_abi_argument_errors(pkg, which):
    """One call per error, fake aligned addresses otherwise: validation runs on the host before anything is launched
    (or, on the CPU twin, touched)."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    f = L.q2048_table_merge
    d, s, c, st = 1 << 30, 1 << 40, 1 << 20, 1 << 21                  # 2^20 slots of 32 B from 2^30 end at 2^30 + 2^25
    NULL, SIZE, ALIGN, RANGE, FLAGS = -1, -2, -3, -6, -7
    assert f(None, 20, s, 20, 1, ADD, 1.0, c, st, None) == NULL
    assert f(d, 20, None, 20, 1, ADD, 1.0, c, st, None) == NULL
    assert f(d, 20, s, 20, 1, ADD, 1.0, None, st, None) == NULL
    assert f(d, 3, s, 20, 1, ADD, 1.0, c, st, None) == SIZE
    assert f(d, 41, s, 20, 1, ADD, 1.0, c, st, None) == SIZE
    assert f(d, 20, s, 3, 1, ADD, 1.0, c, st, None) == SIZE
    assert f(d, 20, s, 41, 1, ADD, 1.0, c, st, None) == SIZE
    assert f(d, 20, s, 20, 0, ADD, 1.0, c, st, None) == SIZE
    assert f(d, 20, s, 20, 3, ADD, 1.0, c, st, None) == SIZE
    assert f(d + 8, 20, s, 20, 1, ADD, 1.0, c, st, None) == ALIGN
    assert f(d, 20, s + 8, 20, 2, ADD, 1.0, c, st, None) == ALIGN
    assert f(d, 20, s, 20, 1, 3, 1.0, c, st, None) == FLAGS
    assert f(d, 20, s, 20, 1, -1, 1.0, c, st, None) == FLAGS
    assert f(d, 20, s, 20, 1, ADD, float("nan"), c, st, None) == RANGE
    assert f(d, 20, s, 20, 1, MAXABS, float("inf"), c, st, None) == RANGE
    assert f(d, 20, s, 20, 1, BLEND, 1.5, c, st, None) == RANGE
    assert f(d, 20, s, 20, 1, BLEND, -0.25, c, st, None) == RANGE
    assert f(d, 20, d, 20, 1, ADD, 1.0, c, st, None) == RANGE                       # src == dst
    assert f(d, 20, d + (32 << 20) - 32, 20, 1, ADD, 1.0, c, st, None) == RANGE     # the last slot of dst is src's first
    assert f(d + (32 << 16) - 32, 20, d, 16, 1, ADD, 1.0, c, st, None) == RANGE     # ... and the other way round
    # the order: NULL before SIZE before ALIGN before FLAGS before RANGE
    assert f(None, 99, s + 8, 20, 3, 9, float("nan"), c, st, None) == NULL
    assert f(d + 8, 99, s, 20, 1, 9, float("nan"), c, st, None) == SIZE
    assert f(d + 8, 20, s, 20, 1, 9, float("nan"), c, st, None) == ALIGN
    assert f(d, 20, s, 20, 1, 9, float("nan"), c, st, None) == FLAGS


# ---------------------------------------------------------------------------------------------
# 2. every mode against the model
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("mode,w", MODES)
def test_modes_equal_the_model(pkg, dev, n, mode, w):
    """Two learners of different seeds: they share the opening states and then diverge, so a merge both combines and
    creates rows."""
    dst = agent_with(pkg, dev, n, trained_rows(pkg, dev, n, 1), 22)
    src = agent_with(pkg, dev, n, trained_rows(pkg, dev, n, 2), 21)
    out, before, other = check_merge(pkg, dst, src, mode, w, f"{mode} w={w} n={n}")
    assert out["combined"] > 0 and out["created"] > 0 and out["dropped"] == 0
    if mode == "blend" and w in (0.0, 1.0):
        # w = 0 keeps every row the destination had, bit for bit; w = 1 makes every shared state the source's row
        ref_k, ref_q = sorted_rows(*(before if w == 0.0 else other))
        gk, gq = sorted_rows(*dst.export_rows())
        pos = locate(gk, ref_k)
        assert np.array_equal(gq[pos].view(np.uint32), ref_q.view(np.uint32))


# ---------------------------------------------------------------------------------------------
# 3. capacities differ; an empty side
# ---------------------------------------------------------------------------------------------
def small_rows(pkg, dev, n, seed):
    return trained_rows(pkg, dev, n, seed, B=256, steps=50)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("caps", [(16, 20), (20, 16)])
def test_capacities_differ(pkg, dev, n, caps):
    src = agent_with(pkg, dev, n, small_rows(pkg, dev, n, 3), caps[0])
    dst = agent_with(pkg, dev, n, small_rows(pkg, dev, n, 4), caps[1])
    out, _, _ = check_merge(pkg, dst, src, "add", 1.0, f"src 2^{caps[0]} into dst 2^{caps[1]}")
    assert out["combined"] > 0 and out["created"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5])
def test_mapped_destination_equals_plain(pkg, n):
    """A destination mapped from physical chunks (the allocator of growing tables) against one from the ordinary
    allocator: the same rows."""
    dev = "cuda:0"
    src = agent_with(pkg, dev, n, small_rows(pkg, dev, n, 3), 16, placement="plain")
    rows = {}
    for placement in ("chunks", "plain"):
        dst = agent_with(pkg, dev, n, small_rows(pkg, dev, n, 4), 20, placement=placement)
        assert dst.placement["kind"] == placement if "kind" in dst.placement else True
        check_merge(pkg, dst, src, "blend", 0.3, placement)
        rows[placement] = sorted_rows(*dst.export_rows())
    assert np.array_equal(rows["chunks"][0], rows["plain"][0])
    assert np.array_equal(rows["chunks"][1].view(np.uint32), rows["plain"][1].view(np.uint32))


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("mode,w", [("add", 0.5), ("blend", 0.3), ("maxabs", 1.0)])
def test_an_empty_side(pkg, dev, n, mode, w):
    rows = small_rows(pkg, dev, n, 3)
    # empty source: the counters stay 0 and the destination keeps every byte
    dst, empty = agent_with(pkg, dev, n, rows, 18), new_agent(pkg, dev, n, 16)
    table = dst.table.clone()
    assert dst.merge_from(empty, mode=mode, weight=w) == {"read": 0, "created": 0, "combined": 0, "dropped": 0}
    sync(dev)
    assert torch.equal(dst.table, table)
    dst.verify_table()
    # empty destination: the result is the source's rows (ADD: scaled by w)
    dst, src = new_agent(pkg, dev, n, 18), agent_with(pkg, dev, n, rows, 16)
    out, _, _ = check_merge(pkg, dst, src, mode, w, "empty destination")
    assert out["created"] == len(rows[1]) and out["combined"] == 0
    if mode != "add":
        sk, sq = sorted_rows(*rows)
        assert_rows_equal(dst.export_rows(), sk, sq, "empty destination takes the rows as they are")


# ---------------------------------------------------------------------------------------------
# 4. K replicas
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_mean_and_maxabs_of_three_replicas(pkg, dev, n):
    reps = [trained_rows(pkg, dev, n, s) for s in (1, 2, 3)]
    third = 1.0 / 3.0
    key_sets, maxabs = [], []
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        # the mean: three ADD merges with w = 1/3 into an empty table; the model accumulates in the same order
        dst = new_agent(pkg, dev, n, 23)
        model = (np.zeros((0, 1 if n == 4 else 2), np.uint64), np.zeros((0, 4), np.float32))
        for i in order:
            out = dst.merge_from(agent_with(pkg, dev, n, reps[i], 21), mode="add", weight=third)
            assert out["dropped"] == 0 and out["read"] == len(reps[i][1])
            mk, mq, created, combined = model_merge(model, reps[i], "add", third)
            assert (out["created"], out["combined"]) == (created, combined)
            model = (mk, mq)
        sync(dev)
        dst.verify_table()
        assert_rows_equal(dst.export_rows(), model[0], model[1], f"mean, order {order}")
        key_sets.append(model[0])
        # the per-action value of largest magnitude over the three
        dst = new_agent(pkg, dev, n, 23)
        for i in order:
            dst.merge_from(agent_with(pkg, dev, n, reps[i], 21), mode="maxabs")
        sync(dev)
        dst.verify_table()
        maxabs.append(sorted_rows(*dst.export_rows()))
    assert all(np.array_equal(k, key_sets[0]) for k in key_sets[1:])          # the key set does not depend on the order
    # MAXABS is the same for every order except where two replicas hold values of equal magnitude and opposite sign
    # (the first one merged wins): those entries are found from the inputs and left out -- there are none here
    u, stack = key_sets[0], []
    for keys, q in reps:
        k, v = sorted_rows(keys, q)
        full = np.zeros((len(u), 4), np.float32)
        full[locate(u, k)] = v
        stack.append(full)
    stack = np.stack(stack)                                                    # [replica, row, action]
    top = np.abs(stack).max(axis=0)
    at_top = np.abs(stack) == top
    tie = ((at_top & (stack > 0)).any(axis=0) & (at_top & (stack < 0)).any(axis=0)).any(axis=1)
    assert tie.mean() == 0.0
    for k, q in maxabs[1:]:
        assert np.array_equal(k, maxabs[0][0])
        assert np.array_equal(q[~tie].view(np.uint32), maxabs[0][1][~tie].view(np.uint32))
    want = np.take_along_axis(stack, np.abs(stack).argmax(axis=0)[None], axis=0)[0]
    assert np.array_equal(maxabs[0][1][~tie].view(np.uint32), want[~tie].view(np.uint32))


# ---------------------------------------------------------------------------------------------
# 5. a destination that is too small
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_full_destination(pkg, dev, n):
    N = pkg._native
    rows = small_rows(pkg, dev, n, 3)
    assert len(rows[1]) > (1 << 12)
    src, dst = agent_with(pkg, dev, n, rows, 16), new_agent(pkg, dev, n, 12)
    with pytest.raises(ValueError, match="too small"):
        dst.merge_from(src)
    sync(dev)
    assert dst.table_size() == 0                                     # refused before anything was launched
    counters = torch.zeros(4, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    N.check(dst._L.q2048_table_merge(dst.table.data_ptr(), 12, src.table.data_ptr(), 16, 1 if n == 4 else 2, ADD, 1.0,
                                     counters.data_ptr(), status.data_ptr(), None), "table_merge")
    sync(dev)
    read, created, combined, dropped = counters.tolist()
    assert dropped > 0 and int(status.item()) & N.STATUS_TABLE_FULL
    assert read == created + combined + dropped == len(rows[1]) and combined == 0
    dst.recount_rows()
    got_k, got_q = sorted_rows(*dst.export_rows())                   # (asserts: no key twice)
    assert len(got_k) == created == 1 << 12                          # the import's probe limit covers the whole table
    sk, sq = sorted_rows(*rows)
    assert np.array_equal(sq[locate(sk, got_k)].view(np.uint32), got_q.view(np.uint32))     # every row kept is a source row
    assert N.claim_timeouts(dst._L) == 0


# ---------------------------------------------------------------------------------------------
# 6. the agent's rules
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_agent_refusals(pkg, dev):
    a4, b4, a5 = new_agent(pkg, dev, 4, 14), new_agent(pkg, dev, 4, 14), new_agent(pkg, dev, 5, 14)
    with pytest.raises(ValueError, match="board size"):
        a4.merge_from(a5)
    with pytest.raises(ValueError):
        a4.merge_from(a4)
    with pytest.raises(ValueError, match="mode"):
        a4.merge_from(b4, mode="mean")
    with pytest.raises(ValueError, match="weight"):
        a4.merge_from(b4, mode="blend", weight=1.5)
    with pytest.raises(ValueError, match="weight"):
        a4.merge_from(b4, weight=float("nan"))
    # a destination whose key set is closed refuses; a frozen SOURCE is only read
    env = pkg.BatchedGame2048Env(512, board_size=4, seed=1, env_id0=0, device=dev)
    frozen = new_agent(pkg, dev, 4, 12, freeze_load=0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(6):
            frozen.fused_rollout(env, 20)
    sync(dev)
    assert frozen.frozen
    with pytest.raises(ValueError, match="closed"):
        frozen.merge_from(b4)
    out, _, _ = check_merge(pkg, new_agent(pkg, dev, 4, 16), frozen, "add", 1.0, "frozen source")
    assert out["created"] == frozen.table_size() > 0


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_growable_destination_grows(pkg, dev, n):
    rows = trained_rows(pkg, dev, n, 1)
    dst = new_agent(pkg, dev, n, "auto", initial_capacity_log2=16, max_capacity_log2=22, prefetch_growth=False)
    assert dst.growable and dst.capacity_log2 == 16 and not dst.growths and 2 * len(rows[1]) > 1 << 16
    src = agent_with(pkg, dev, n, rows, 21)
    out, _, _ = check_merge(pkg, dst, src, "blend", 1.0, "growable destination")
    assert out["created"] == len(rows[1])
    assert dst.growths and dst.growths[-1]["to_log2"] == dst.capacity_log2
    assert 2 * len(rows[1]) <= (1 << dst.capacity_log2)


@pytest.mark.parametrize("dev", DEVICES)
def test_summaries_end_with_a_merge_and_the_closed_rollout_agrees(pkg, dev):
    """A 4x4 table that carries line summaries is merged into: the agent stops believing them.  The merged table then
    closes its key set (the union passes freeze_load), the summaries are written again for the new key set, and a
    rollout on it equals the same rollout on an agent that imported the model's rows.  Private rows per env, so that
    the rollout is a function of its inputs on the GPU too."""
    B, tables = 256, []
    for seed in (3, 4):
        env = pkg.BatchedGame2048Env(B, board_size=4, seed=seed, env_id0=0, device=dev)
        agent = new_agent(pkg, dev, 4, 17, seed=seed, independent=True)
        agent.fused_rollout(env, 50)
        sync(dev)
        tables.append(agent.export_rows())
    a_rows, b_rows = tables
    mk, mq, created, _ = model_merge(a_rows, b_rows, "add", 0.5)
    cap = int(np.ceil(np.log2((len(a_rows[1]) + len(b_rows[1])) / 0.9)))
    assert len(mk) >= 0.2 * (1 << cap) and created > 0
    merged = agent_with(pkg, dev, 4, a_rows, cap, freeze_load=0.2, independent=True)
    pkg._native.check(merged._L.q2048_table_summarise(merged.table.data_ptr(), cap, None), "table_summarise")
    merged._summarised = True                             # the slots carry summaries of the key set before the merge
    merged.merge_from(agent_with(pkg, dev, 4, b_rows, 17, independent=True), mode="add", weight=0.5)
    assert not merged._summarised and merged._side is None
    merged.verify_table()
    assert_rows_equal(merged.export_rows(), mk, mq, "merge into a summarised table")
    model = agent_with(pkg, dev, 4, (mk[:, 0], mq), cap, freeze_load=0.2, independent=True)
    ends = []
    for agent in (merged, model):
        env = pkg.BatchedGame2048Env(B, board_size=4, seed=3, env_id0=0, device=dev)
        agent.seed, agent.ctr = 3, 0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(3):
                agent.fused_rollout(env, 20)
        sync(dev)
        assert agent.frozen and agent._summarised and agent.check_status() == 0
        ends.append((env.boards.clone(), env.aux.clone(), rows_of(agent), agent.stats()))
    assert torch.equal(ends[0][0], ends[1][0]) and torch.equal(ends[0][1], ends[1][1])
    assert torch.equal(ends[0][2], ends[1][2])
    assert ends[0][3]["drops"] == ends[1][3]["drops"] > 0 and ends[0][3]["inserts"] == 0


# ---------------------------------------------------------------------------------------------
# 7. the script
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_merge_tables_script(pkg, dev, tmp_path):
    device = "cpu" if dev == "cpu" else "cuda"
    py = lambda script, *a: subprocess.run([sys.executable, os.path.join(REPO, script), "--device", device, *a],   # noqa: E731
                                           capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    for seed in (1, 2):
        p = py("train.py", "--num-envs", "512", "--steps-per-launch", "32", "--episodes", "3", "--max-steps", "96",
               "--capacity-log2", "18", "--seed", str(seed), "--save", f"q{seed}.pt", "--log", f"log{seed}.csv")
        assert p.returncode == 0, p.stderr[-2000:]
    p = py("merge_tables.py", "--mode", "mean", "--out", "merged.pt", "q1.pt", "q2.pt")
    assert p.returncode == 0, p.stderr[-2000:]
    report = json.loads(p.stdout.strip().splitlines()[-1])
    a, b, m = (torch.load(tmp_path / f, map_location="cpu", weights_only=False) for f in ("q1.pt", "q2.pt", "merged.pt"))
    empty = (np.zeros((0, 1), np.uint64), np.zeros((0, 4), np.float32))
    k1, q1, c1, _ = model_merge(empty, (a["keys"], a["q"]), "add", 0.5)
    mk, mq, c2, s2 = model_merge((k1, q1), (b["keys"], b["q"]), "add", 0.5)
    assert_rows_equal((m["keys"], m["q"]), mk, mq, "merge_tables.py --mode mean")
    assert report["rows_out"] == len(mk) == len(np.union1d(a["keys"], b["keys"])) and report["rows_in"] == [len(a["q"]), len(b["q"])]
    assert report["merges"] == [{"read": c1, "created": c1, "combined": 0, "dropped": 0},
                                {"read": c2 + s2, "created": c2, "combined": s2, "dropped": 0}]
    assert s2 > 0 and c2 > 0
    assert m["lr"] == a["lr"] and m["schedule"] == a["schedule"] and m["ctr"] == max(a["ctr"], b["ctr"])
    assert torch.equal(m["stats_i"], a["stats_i"] + b["stats_i"]) and torch.equal(m["stats_f"], a["stats_f"] + b["stats_f"])
    # ... and it loads: evaluation, and a resumed run
    p = py("evaluate.py", "--model", "merged.pt", "--num-envs", "256", "--episodes", "1", "--max-steps", "64")
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1])["rows"] == len(mk)
    p = py("train.py", "--num-envs", "512", "--steps-per-launch", "32", "--episodes", "4", "--max-steps", "32",
           "--capacity-log2", "18", "--seed", "1", "--resume", "merged.pt", "--log", "log3.csv")
    assert p.returncode == 0, p.stderr[-2000:]
    # mixed board sizes are refused
    p = py("train.py", "--num-envs", "64", "--steps-per-launch", "8", "--episodes", "1", "--max-steps", "8", "--board-size", "5",
           "--capacity-log2", "16", "--save", "q5.pt", "--log", "log5.csv")
    assert p.returncode == 0, p.stderr[-2000:]
    p = py("merge_tables.py", "--out", "bad.pt", "q1.pt", "q5.pt")
    assert p.returncode != 0 and "board size" in p.stderr and not (tmp_path / "bad.pt").exists()


# ---------------------------------------------------------------------------------------------
# 8. at size
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_merge_at_size(pkg):
    """Two learners of 2^20 envs x 64 steps in 2^28-slot tables, summed: the counters' identity, the table check, and
    200 000 sampled states against the model through q_values."""
    dev, B, cap = "cuda:0", 1 << 20, 28
    agents = []
    for seed in (1, 2):
        env = pkg.BatchedGame2048Env(B, board_size=4, seed=seed, env_id0=0, device=dev)
        agent = new_agent(pkg, dev, 4, cap, seed=seed, placement="plain")
        agent.fused_rollout(env, 64)
        agents.append(agent)
        del env
    a, b = agents
    torch.cuda.synchronize()
    rows_a, rows_b = a.verify_table()["rows"], b.verify_table()["rows"]
    # 100 000 states of each table, read from randomly chosen occupied slots
    gen = torch.Generator(device=dev).manual_seed(5)
    keys = []
    for agent in agents:
        slots = torch.randint(0, 1 << cap, (1 << 21,), generator=gen, device=dev)
        k = agent.table.view(torch.int64).reshape(-1, 4)[slots, 0]
        k = torch.unique(k[k != 0])
        assert k.numel() >= 100000
        keys.append(k[torch.randperm(k.numel(), generator=gen, device=dev)[:100000]])
    keys = torch.unique(torch.cat(keys))
    boards = ((keys[:, None] >> (4 * torch.arange(16, device=dev))[None, :]) & 15).to(torch.uint8)
    qa, fa = a.q_values(boards, return_found=True)
    qb, fb = b.q_values(boards, return_found=True)
    assert bool((fa | fb).all()) and int((fa & fb).sum()) > 0
    want = torch.where((fa & fb)[:, None], qa + qb, torch.where(fa[:, None], qa, qb))   # ADD, w = 1: 1 * q is q
    out = a.merge_from(b, mode="add", weight=1.0)
    torch.cuda.synchronize()
    assert out["dropped"] == 0 and out["read"] == out["created"] + out["combined"] == rows_b
    assert out["combined"] > 0 and out["created"] > 0
    assert a.verify_table()["rows"] == rows_a + out["created"]
    assert pkg._native.claim_timeouts(a._L) == 0 and a.check_status() == 0
    got, found = a.q_values(boards, return_found=True)
    assert bool(found.all())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
