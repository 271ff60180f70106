"""Line summaries of 5x5 tables with a closed key set: the side array (q2048_table_summarise_side,
q2048_rollout_opts.line_summary, Q2048_FLAG_LINE_SUMMARY on n = 5).

Same results as the slot-by-slot probe -- same slot, same row, same drops, same visit rows -- decided from one
8-byte word per 128-byte line that lives beside the table.  Every test runs on the CPU twin ("cpu": its 5x5 fused
rollout decides its closed-key-set lookups through the decode function the kernel uses) and on the GPU."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]


def mix64(x):
    """q2048::mix64 (csrc/q2048_core.hpp) on uint64 arrays, restated for the checks."""
    x = x * np.uint64(0x9E3779B97F4A7C15)
    x = x ^ (x >> np.uint64(29))
    x = x * np.uint64(0xBF58476D1CE4E5B9)
    return x ^ (x >> np.uint64(32))


def expected_words(table, key_words):
    """The side array of a raw table, recomputed from its key words: uint64 [lines]."""
    raw = table.cpu().numpy().view(np.uint64).reshape(-1, 4, 4)               # [line, slot, word]
    k0, k1 = raw[:, :, 0], raw[:, :, 3]
    with np.errstate(over="ignore"):
        h = mix64(k0 ^ (k1 * np.uint64(0x9E3779B97F4A7C15))) if key_words == 2 else mix64(k0)
    fp = np.where(k0 != 0, ((h >> np.uint64(48)) & np.uint64(0xFFFF)) | np.uint64(1), np.uint64(0))
    words = np.zeros(len(raw), np.uint64)
    for r in range(4):
        words |= fp[:, r] << np.uint64(16 * r)
    return words, k0


def side_words(agent):
    return agent._side.cpu().numpy().view(np.uint64)


def key_words_of(table):
    raw = table.cpu().numpy().view(np.uint64).reshape(-1, 4)
    return raw[:, 0].copy(), raw[:, 3].copy()


def rows_of(agent):
    """The table as its rows -- the occupied slots' 32 bytes, sorted -- for comparing two runs bit for bit.  WHERE a
    row lies is decided while rows are created: on the GPU lanes race for the slots of a shared line, so two runs of
    the same learning phase may place the same rows differently (with or without summaries); what the rows hold is
    the run's result."""
    t = agent.table.view(torch.int64).reshape(-1, 4)
    return torch.unique(t[t[:, 0] != 0], dim=0)


def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def mk5(pkg, dev, B, cap, seed=5, id0=900, eps=0.3, **kw):
    env = pkg.BatchedGame2048Env(B, board_size=5, seed=seed, env_id0=id0, device=dev)
    kw.setdefault("freeze_load", None)
    agent = pkg.BatchedQLearningAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=eps,
                                      capacity_log2=cap, seed=seed, env_id0=id0, device=dev, board_size=5, **kw)
    return env, agent


# ---------------------------------------------------------------------------------------------
# 1. ABI
# ---------------------------------------------------------------------------------------------
def test_both_libraries_export_the_side_pass(pkg):
    import os

    N = pkg._native
    assert hasattr(N.host_lib(), "q2048_table_summarise_side")
    assert "q2048_table_summarise_side" in N._SIGNATURES
    if os.path.exists(N.LIB_PATH):                    # (a host without hipcc has only the CPU twin)
        assert hasattr(N.lib(), "q2048_table_summarise_side")
    assert N.lib_for(torch.device("cpu")).q2048_abi_version() == 7


def test_rollout_opts_layout(pkg):
    N = pkg._native
    assert C.sizeof(N.RolloutOpts) == 64
    assert N.RolloutOpts._fields_[-1][0] == "line_summary" and N.RolloutOpts.line_summary.offset == 56
    assert N.RolloutOpts().size == 64 and not N.RolloutOpts().line_summary


@pytest.mark.parametrize("dev", DEVICES)
def test_abi_argument_errors(pkg, dev):
    N = pkg._native
    L = N.lib_for(torch.device(dev))
    env, agent = mk5(pkg, dev, 64, 12)
    side = torch.zeros(1 << 10, dtype=torch.int64, device=dev)
    t, s, cap = agent.table.data_ptr(), side.data_ptr(), agent.capacity_log2
    f = L.q2048_table_summarise_side
    assert f(None, cap, 2, s, None) == -1 and f(t, cap, 2, None, None) == -1          # Q2048_ERR_NULL
    assert f(t, cap, 0, s, None) == -2 and f(t, cap, 3, s, None) == -2                  # key_words: Q2048_ERR_SIZE
    assert f(t, cap, 2, s + 4, None) == -3                                              # Q2048_ERR_ALIGN
    assert f(t, 3, 2, s, None) == -2 and f(t, 41, 2, s, None) == -2                     # cap_log2 as check_table
    assert f(t + 8, cap, 2, s, None) == -3
    assert f(None, cap, 0, s + 4, None) == -1 and f(t, cap, 0, s + 4, None) == -2       # the order: NULL, SIZE, ALIGN
    assert f(t, cap, 2, s, None) == 0 and f(t, cap, 1, s, None) == 0
    sync(dev)

    def call(opts, flags=N.FLAG_NO_NEW_ROWS | N.FLAG_LINE_SUMMARY):
        return L.q2048_fused_rollout_opts(
            env.boards.data_ptr(), env.aux.data_ptr(), t, cap, 64, 5, 1, 0.5, 0.1, 0.9, 5, 900, 0, flags,
            agent.stats_i.data_ptr(), agent.stats_f.data_ptr(), agent.status.data_ptr(), C.byref(opts), None)

    old = N.RolloutOpts(); old.size = 56              # the layout shipped before `line_summary`: accepted
    assert call(old) == 0
    for size in (8, 60, 72):
        bad = N.RolloutOpts(); bad.size = size
        assert call(bad) == -2, size
    assert f(t, cap, 2, s, None) == 0
    assert call(N.RolloutOpts(line_summary=s)) == 0
    assert call(N.RolloutOpts(line_summary=s + 4)) == -3
    sync(dev)
    assert agent.check_status() == 0


# ---------------------------------------------------------------------------------------------
# 2. format
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [64, 192])
def test_side_array_format_5x5(pkg, dev, B):
    """Every word of the side array against the fingerprints recomputed from the raw table's two key words; the pass
    writes nothing to the table; an empty line is 0."""
    N = pkg._native
    env, agent = mk5(pkg, dev, B, 14)
    agent.fused_rollout(env, 60)
    assert not agent.side_summarised and agent._side is None
    # the pass by hand: the table is byte-identical afterwards
    before = agent.table.clone()
    buf = torch.full((1 << 12,), -1, dtype=torch.int64, device=dev)
    N.check(agent._L.q2048_table_summarise_side(agent.table.data_ptr(), 14, 2, buf.data_ptr(), None), "side")
    sync(dev)
    assert torch.equal(before, agent.table)
    want, k0 = expected_words(agent.table, 2)
    assert np.array_equal(buf.cpu().numpy().view(np.uint64), want)
    empty = ~k0.any(axis=1)
    assert empty.sum() > 100 and (~empty).sum() > 1000 and not want[empty].any() and want[~empty].all()
    # ... and by the agent, at the first launch after the key set closed
    keys_before = key_words_of(agent.table)
    agent.frozen = True
    agent.fused_rollout(env, 20)
    assert agent.side_summarised and not agent._summarised and agent._side.numel() == 1 << 12
    keys_after = key_words_of(agent.table)
    assert np.array_equal(keys_before[0], keys_after[0]) and np.array_equal(keys_before[1], keys_after[1])
    assert np.array_equal(side_words(agent), want)
    assert agent.stats()["drops"] > 0 and agent.check_status() == 0 and N.claim_timeouts(agent._L) == 0


@pytest.mark.parametrize("dev", DEVICES)
def test_side_array_key_words_1_equals_the_in_slot_summaries(pkg, dev):
    N = pkg._native
    env = pkg.BatchedGame2048Env(128, seed=5, device=dev)
    agent = pkg.BatchedQLearningAgent(100, exploration_rate=0.3, capacity_log2=14, seed=5, device=dev, freeze_load=None)
    agent.fused_rollout(env, 60)
    buf = torch.zeros(1 << 12, dtype=torch.int64, device=dev)
    N.check(agent._L.q2048_table_summarise_side(agent.table.data_ptr(), 14, 1, buf.data_ptr(), None), "side")
    N.check(agent._L.q2048_table_summarise(agent.table.data_ptr(), 14, None), "summarise")
    sync(dev)
    got = buf.cpu().numpy().view(np.uint64)
    in_slots = agent.table.cpu().numpy().view(np.uint64).reshape(-1, 4, 4)[:, :, 3]
    assert got.any() and all(np.array_equal(in_slots[:, r], got) for r in range(4))
    assert np.array_equal(got, expected_words(agent.table, 1)[0])


# ---------------------------------------------------------------------------------------------
# 3. same results
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_private_rows_against_the_oracle_and_against_slot_by_slot(pkg, O, dev):
    """The 5x5 twin of the private-rows part of test_line_summaries_of_a_closed_key_set: 192 envs with private rows,
    60 learning steps, the key set closes, 120 steps in two launches -- every oracle row, every board, every drop; and
    the run with `line_summaries = False` on the same path is bit-identical."""
    B, k1, k2, seed, id0, eps, lr, gamma = 192, 60, 120, 5, 900, 0.1, 0.1, 0.95
    runs = {}
    for summaries in (True, False):
        env, agent = mk5(pkg, dev, B, 17, seed=seed, id0=id0, eps=eps, independent=True)
        agent.line_summaries = summaries
        agent.fused_rollout(env, k1)
        agent.frozen = True
        agent.fused_rollout(env, k2 // 3)
        agent.fused_rollout(env, k2 - k2 // 3)
        assert agent.side_summarised == summaries and not agent._summarised
        runs[summaries] = (env, agent)
    env, agent = runs[True]
    envs = O.envs_init(B, 5, seed, id0)
    drops = 0
    for i in range(B):
        oa = O.Agent(100, 4, lr, gamma, eps, n=5)
        O.rollout(envs[i:i + 1], oa, k1, seed, id0 + i, 0)
        oa.freeze()
        O.rollout(envs[i:i + 1], oa, k2, seed, id0 + i, k1)
        drops += oa.drops
        keys, vals = oa.dump()
        boards = torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint8)).to(dev)
        got, found = agent.q_values(boards, env_id=id0 + i, return_found=True)
        assert bool(found.all()) and np.allclose(got.cpu().numpy(), vals, rtol=1e-5, atol=1e-6), i
    assert np.array_equal(env.boards.cpu().numpy(), envs["board"][:, :25])
    assert agent.stats()["drops"] == drops > 0 and agent.check_status() == 0
    env0, agent0 = runs[False]
    assert torch.equal(rows_of(agent), rows_of(agent0)) and torch.equal(env.boards, env0.boards)
    assert torch.equal(env.aux, env0.aux)
    assert torch.equal(agent.stats_i, agent0.stats_i) and torch.equal(agent.stats_f, agent0.stats_f)


# ---------------------------------------------------------------------------------------------
# 4. the array is what decides
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_the_side_array_decides_the_lookups(pkg, dev):
    """With the side array zeroed by hand every line reads as empty: each of the launch's B * k lookups is absent --
    B * k drops, not one table byte changes.  (No row cache: no launch starts from a carried table row.)  After a
    launch with the key set open the array is written again and the lookups find their rows again."""
    B, k = 128, 6
    env, agent = mk5(pkg, dev, B, 14, row_cache=False)
    agent.fused_rollout(env, 60)
    agent.frozen = True
    agent.fused_rollout(env, k)
    assert agent.side_summarised
    d0 = agent.stats()["drops"]
    assert 0 < d0 < B * k
    agent._side.zero_()
    before = agent.table.clone()
    agent.fused_rollout(env, k)
    d1 = agent.stats()["drops"]
    assert d1 - d0 == B * k
    assert torch.equal(before, agent.table)
    agent.frozen = False
    agent.fused_rollout(env, 2)
    assert not agent.side_summarised
    agent.frozen = True
    d2 = agent.stats()["drops"]
    agent.fused_rollout(env, k)
    assert agent.side_summarised and np.array_equal(side_words(agent), expected_words(agent.table, 2)[0])
    assert side_words(agent).any() and agent.stats()["drops"] - d2 < B * k
    assert agent.check_status() == 0


# ---------------------------------------------------------------------------------------------
# 5. lifecycle
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_validity_follows_the_key_set(pkg, dev):
    env, agent = mk5(pkg, dev, 128, 15)
    agent.fused_rollout(env, 40)
    agent.frozen = True
    agent.fused_rollout(env, 4)
    assert agent.side_summarised
    agent.fused_rollout(env, 4, learn=False)          # evaluation and play-only neither use nor end them
    agent.fused_rollout(env, 4, play_only=True)
    assert agent.side_summarised
    agent.frozen = False                              # a launch with the key set open
    agent.fused_rollout(env, 2)
    assert not agent.side_summarised
    agent.frozen = True
    agent.fused_rollout(env, 2)
    assert agent.side_summarised
    keys, q = agent.export_rows()                     # import_rows
    other = mk5(pkg, dev, 128, 15)[1]
    other.frozen = True
    other._side = torch.zeros(1 << 13, dtype=torch.int64, device=dev)
    other.import_rows(keys, q)
    assert not other.side_summarised
    assert "line_summary" not in agent.state_dict() and not any("side" in k for k in agent.state_dict())
    agent.load_state_dict(agent.state_dict())         # load_state_dict
    assert not agent.side_summarised and not agent.frozen
    agent.frozen = True
    agent.fused_rollout(env, 2)
    assert agent.side_summarised and np.array_equal(side_words(agent), expected_words(agent.table, 2)[0])
    assert agent.check_status() == 0


@pytest.mark.parametrize("dev", DEVICES)
def test_frozen_checkpoint_resumes_bit_identically(pkg, dev):
    """A checkpoint taken with the key set closed resumes to the uninterrupted run, summaries on in both (the side
    array is not part of the checkpoint: the resumed agent writes its own at its first frozen launch)."""
    B = 200

    def mk():
        return mk5(pkg, dev, B, 16, seed=9, id0=4242, eps=0.05, independent=True)

    e1, a1 = mk()
    a1.fused_rollout(e1, 30)
    a1.frozen = True
    a1.fused_rollout(e1, 30)
    assert a1.side_summarised
    sd_env, sd = e1.state_dict(), a1.state_dict(compact=False)
    a1.fused_rollout(e1, 40)
    e2, a2 = mk()
    e2.load_state_dict(sd_env); a2.load_state_dict(sd)
    assert not a2.side_summarised
    a2.frozen = True
    a2.fused_rollout(e2, 40)
    assert a2.side_summarised and np.array_equal(side_words(a1), side_words(a2))
    assert torch.equal(a1.table, a2.table) and torch.equal(e1.boards, e2.boards) and torch.equal(e1.aux, e2.aux)
    assert torch.equal(a1.stats_i, a2.stats_i) and torch.equal(a1.stats_f, a2.stats_f)
    assert a1.stats()["drops"] > 0 and a2.check_status() == 0


@pytest.mark.parametrize("dev", DEVICES)
def test_growing_table_ends_with_an_array_of_its_final_capacity(pkg, dev):
    B, S = 4096, 8
    env = pkg.BatchedGame2048Env(B, board_size=5, seed=3, device=dev)
    agent = pkg.BatchedQLearningAgent(100, exploration_rate=0.9, capacity_log2="auto", initial_capacity_log2=16,
                                      max_capacity_log2=18, seed=3, device=dev, board_size=5, freeze_load=0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(24):
            agent.fused_rollout(env, S)
            assert agent.side_summarised == agent.frozen
    agent.finish_growth()
    assert agent.frozen and agent.capacity_log2 == 18 and agent._side.numel() == 1 << 16
    check = agent.verify_table()
    assert check["rows"] == agent.frozen_at["rows"] and agent.stats()["drops"] > 0 and agent.check_status() == 0
    assert np.array_equal(side_words(agent), expected_words(agent.table, 2)[0])


# ---------------------------------------------------------------------------------------------
# 6. no room for the array
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_allocation_failure_falls_back_to_slot_by_slot(pkg, dev, monkeypatch):
    calls = []

    def refuse(self, words):
        calls.append(words)
        raise torch.OutOfMemoryError("no room (test)")

    runs = {}
    for patched in (True, False):
        env, agent = mk5(pkg, dev, 128, 15, independent=True)
        if patched:
            monkeypatch.setattr(type(agent), "_alloc_side_summaries", refuse)
        else:
            agent.line_summaries = False
        agent.fused_rollout(env, 40)
        agent.frozen = True
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for _ in range(3):
                agent.fused_rollout(env, 10)
        if patched:
            assert calls == [1 << 13] and not agent.side_summarised
            assert sum("line summaries" in str(w.message) for w in caught) == 1
            monkeypatch.undo()
        else:
            assert not caught
        runs[patched] = (env, agent)
    (e1, a1), (e0, a0) = runs[True], runs[False]
    assert torch.equal(rows_of(a1), rows_of(a0)) and torch.equal(e1.boards, e0.boards) and torch.equal(e1.aux, e0.aux)
    assert torch.equal(a1.stats_i, a0.stats_i) and a1.stats()["drops"] > 0 and a1.check_status() == 0


# ---------------------------------------------------------------------------------------------
# 7. full size (GPU only)
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1 << 20, (1 << 20) + 77])
def test_full_size_summaries_on_equal_off(pkg, B):
    """2^20 (+77: a ragged last block) envs with private rows on a 2^27-slot table, sized like
    test_full_size_1m_lanes_closed_key_set[5-27]: one learning launch, the key set closes, three 16-step launches --
    summaries on == off bit for bit."""
    dev, S = "cuda:0", 16
    runs = {}
    for summaries in (True, False):
        env = pkg.BatchedGame2048Env(B, board_size=5, seed=33, env_id0=5, device=dev)
        agent = pkg.BatchedQLearningAgent(1000, learning_rate=0.1, discount_factor=0.99, exploration_rate=0.2,
                                          capacity_log2=27, seed=33, env_id0=5, device=dev, independent=True,
                                          board_size=5, freeze_load=None)
        agent.line_summaries = summaries
        agent.fused_rollout(env, S)
        rows1 = agent.table_size()
        agent.frozen = True
        for _ in range(3):
            agent.fused_rollout(env, S)
        assert agent.side_summarised == summaries
        st = agent.stats()
        assert st["steps"] == 4 * B * S and st["inserts"] == rows1 == agent.table_size() and st["drops"] > B
        assert agent.check_status() == 0 and pkg._native.claim_timeouts() == 0
        runs[summaries] = (env.boards.cpu(), env.aux.cpu(), agent.stats_i.cpu(), agent.stats_f.cpu(), rows_of(agent))
        if summaries:
            assert agent._side.numel() == 1 << 25
        del env, agent
    on, off = runs[True], runs[False]
    for a, b in zip(on[:3], off[:3]):                 # boards, aux, the integer statistics
        assert torch.equal(a, b)
    # the float statistics are sums of 6.7e7 rewards added by atomics in the order blocks happen to finish: two runs of
    # one build differ in the last bits.  Bound: n * 2^-53 = 7.5e-9 relative (all rewards of one sign at worst)
    assert torch.allclose(on[3], off[3], rtol=1e-8, atol=0.0)
    assert len(on[4]) > B and torch.equal(on[4], off[4])      # every row of the two tables, compared on the device
