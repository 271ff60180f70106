"""Symmetry folding: Q2048_FLAG_SYMMETRIC, q2048_canonicalize, BatchedQLearningAgent(symmetric=True),
`train.py --symmetric`.

A folded table holds one row for the eight mirror images of a board, keyed by the image with the smallest packed key
(include/q2048.h: images, tie rule, action table).  The model every test compares with is numpy written here from
that definition -- np.rot90 / np.fliplr, the nibble packing, min -- plus the oracle's draws for the draw contract;
all comparisons are exact.  Every test runs on the CPU twin and on the GPU."""
import ctypes as C
import importlib
import json
import math
import os
import subprocess
import sys
import types
import warnings

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
FLAG_SYMMETRIC = 1 << 26
SHIFTS = (4 * np.arange(16, dtype=np.uint64)).reshape(4, 4)


def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# the numpy model (include/q2048.h, Q2048_FLAG_SYMMETRIC)
# ---------------------------------------------------------------------------------------------
def images(b):
    """The eight images of boards b [M, 4, 4]: g = 0..3 np.rot90(b, g); g = 4..7 np.rot90(np.fliplr(b), g - 4)."""
    f = b[:, :, ::-1]                                                   # np.fliplr of every board
    return [np.rot90(b, g, axes=(1, 2)) for g in range(4)] + [np.rot90(f, g, axes=(1, 2)) for g in range(4)]


def pack(b):
    """The packed key: cell 4r + c in nibble 4r + c (low nibble of the tile)."""
    return ((b.astype(np.uint64) & np.uint64(15)) << SHIFTS[None]).sum(axis=(1, 2), dtype=np.uint64)


def canon(boards):
    """boards uint8 [M, 16] -> (canonical images uint8 [M, 16], g uint8 [M], canonical keys uint64 [M])."""
    b = np.asarray(boards, dtype=np.uint8).reshape(-1, 4, 4)
    img = images(b)
    keys = np.stack([pack(x) for x in img])                             # [8, M]
    g = np.argmin(keys, axis=0)                                         # the first minimum: the smallest g on a tie
    out = np.stack(img)[g, np.arange(len(b))]
    return out.reshape(-1, 16).copy(), g.astype(np.uint8), keys.min(axis=0)


def unpack(keys):
    keys = np.asarray(keys, dtype=np.uint64)
    return ((keys[:, None] >> (4 * np.arange(16, dtype=np.uint64))[None]) & np.uint64(15)).astype(np.uint8)


def pi(g, a):
    """pi_g(a): move(image_g(b), pi_g(a)) == image_g(move(b, a))."""
    g, a = np.asarray(g, dtype=np.int64), np.asarray(a, dtype=np.int64)
    return np.where(g < 4, (a - g) & 3, (2 - a - (g - 4)) & 3)


def env_rows(q_canon, g):
    """Rows of the canonical images [M, 4] in the env's frame: Q_env[a] = Q_canon[pi_g(a)]."""
    idx = np.stack([pi(g, a) for a in range(4)], axis=1)
    return np.take_along_axis(q_canon, idx, axis=1)


def random_boards(M, seed):
    """Sparse and full boards, tiles up to 2^15."""
    rng = np.random.default_rng(seed)
    b = rng.integers(1, 16, size=(M, 16), dtype=np.uint8)
    density = np.array([0.1, 0.3, 0.6, 1.0, 1.0])[rng.integers(0, 5, M)]      # two in five boards are full
    b[rng.random((M, 16)) >= density[:, None]] = 0
    return b


def one_move_board(action):
    g = np.array([[1 + ((r + c) & 1) for c in range(4)] for r in range(4)], dtype=np.uint8)
    if action == 0: g[:, 0] = 0
    if action == 2: g[:, 3] = 0
    if action == 1: g[0, :] = 0
    if action == 3: g[3, :] = 0
    return g.reshape(-1)


def canonicalize(pkg, dev, boards, alias=False, want_g=True):
    """q2048_canonicalize through the ABI on `dev`."""
    L = pkg._native.lib_for(torch.device(dev))
    t = torch.from_numpy(np.array(boards, dtype=np.uint8)).to(dev)      # (a copy: in place must not touch the caller's)
    out = t if alias else torch.full_like(t, 0xEE)
    g = torch.full((len(boards),), 0xEE, dtype=torch.uint8, device=dev)
    code = L.q2048_canonicalize(t.data_ptr(), len(boards), 4, out.data_ptr(), g.data_ptr() if want_g else None, None)
    assert code == 0
    sync(dev)
    return out.cpu().numpy(), g.cpu().numpy()


def legal(pkg, dev, boards):
    L = pkg._native.lib_for(torch.device(dev))
    t = torch.from_numpy(np.ascontiguousarray(boards, dtype=np.uint8)).to(dev)
    m = torch.empty(len(boards), dtype=torch.uint8, device=dev)
    assert L.q2048_legal_moves(t.data_ptr(), len(boards), 4, m.data_ptr(), None) == 0
    sync(dev)
    return m.cpu().numpy()


def make(pkg, dev, B, symmetric, independent=False, cap=16, seed=11, id0=500, eps=0.3, profile="shaped",
         reset_shaping_state=False, **kw):
    env = pkg.BatchedGame2048Env(B, 4, dev, seed, id0, profile=profile, reset_shaping_state=reset_shaping_state)
    agent = pkg.BatchedQLearningAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=eps,
                                      capacity_log2=cap, seed=seed, env_id0=id0, device=dev, independent=independent,
                                      placement="plain", symmetric=symmetric, **kw)
    return env, agent


def twin_of(pkg, env):
    other = pkg.BatchedGame2048Env(env.num_envs, 4, env.device, env.seed, env.env_id0, profile=env.profile,
                                   reset_shaping_state=env.reset_shaping_state)
    other.load_state_dict(env.state_dict())
    return other


def rows_of(agent):
    """The table as a set of (key, four float32 bit patterns)."""
    k, q = agent.export_rows()
    return set(zip(k.tolist(), map(tuple, q.view(np.uint32).tolist())))


class _quiet:
    """The freeze warning of a table that fills up is expected here."""

    def __enter__(self):
        self._c = warnings.catch_warnings()
        self._c.__enter__()
        warnings.simplefilter("ignore")

    def __exit__(self, *exc):
        return self._c.__exit__(*exc)


# ---------------------------------------------------------------------------------------------
# 1. the canonical form against the numpy model
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_canonical_form_against_numpy(pkg, dev):
    boards = random_boards(4096, 1)
    assert boards.max() == 15 and (boards != 0).all(axis=1).sum() > 1024 and ((boards != 0).sum(axis=1) <= 3).sum() > 256
    want_b, want_g, want_k = canon(boards)
    got_b, got_g = canonicalize(pkg, dev, boards)
    assert np.array_equal(got_b, want_b) and np.array_equal(got_g, want_g)
    assert set(np.unique(want_g)) == set(range(8))                      # every image occurs as the canonical one
    assert np.array_equal(pack(got_b.reshape(-1, 4, 4)), want_k)
    # the eight images of 64 boards: one canonical image, and sym_out composes to it
    for g, img in enumerate(images(boards[:64].reshape(-1, 4, 4))):
        flat = np.ascontiguousarray(img).reshape(-1, 16)
        out_b, out_g = canonicalize(pkg, dev, flat)
        assert np.array_equal(out_b, want_b[:64]), g
        again = np.stack(images(img))[out_g, np.arange(64)].reshape(-1, 16)
        assert np.array_equal(again, want_b[:64]), g
    # aliased output, outputs left out, B = 1 and B = 77
    for B in (1, 77):
        in_place, g_alias = canonicalize(pkg, dev, boards[:B], alias=True)
        assert np.array_equal(in_place, want_b[:B]) and np.array_equal(g_alias, want_g[:B])
        only_b, untouched = canonicalize(pkg, dev, boards[:B], want_g=False)
        assert np.array_equal(only_b, want_b[:B]) and (untouched == 0xEE).all()
    L = pkg._native.lib_for(torch.device(dev))
    t = torch.from_numpy(boards[:77].copy()).to(dev)
    g = torch.zeros(77, dtype=torch.uint8, device=dev)
    assert L.q2048_canonicalize(t.data_ptr(), 77, 4, None, g.data_ptr(), None) == 0     # boards_out may be NULL
    sync(dev)
    assert np.array_equal(g.cpu().numpy(), want_g[:77]) and np.array_equal(t.cpu().numpy(), boards[:77])


@pytest.mark.parametrize("dev", DEVICES)
def test_stabiliser_boards_take_the_smallest_g(pkg, dev):
    rng = np.random.default_rng(5)
    uniform = np.full((4, 4), 3, dtype=np.uint8)
    a = rng.integers(0, 16, (4, 4), dtype=np.uint8)
    transpose_sym = np.triu(a) + np.triu(a, 1).T
    mirror_lr = np.concatenate([a[:, :2], a[:, 1::-1]], axis=1)
    mirror_ud = np.concatenate([a[:2], a[1::-1]], axis=0)
    anti = np.rot90(transpose_sym)                                       # symmetric in the other diagonal
    half_turn = np.concatenate([a[:2], np.rot90(a[:2], 2)], axis=0)
    empty = np.zeros((4, 4), dtype=np.uint8)
    hand = np.stack([uniform, transpose_sym, mirror_lr, mirror_ud, anti, half_turn, empty]).astype(np.uint8)
    assert np.array_equal(transpose_sym, transpose_sym.T) and np.array_equal(mirror_lr, mirror_lr[:, ::-1])
    # every image of every hand-made board, so that ties are met at every g
    every = np.concatenate([np.ascontiguousarray(x).reshape(-1, 16) for x in images(hand)])
    want_b, want_g, _ = canon(every)
    got_b, got_g = canonicalize(pkg, dev, every)
    assert np.array_equal(got_b, want_b) and np.array_equal(got_g, want_g)
    keys = np.stack([pack(x) for x in images(every.reshape(-1, 4, 4))])
    ties = (keys == keys.min(axis=0)[None]).sum(axis=0)
    assert (ties >= 2).all() and ties.max() == 8                        # each has a stabiliser; the uniform board all 8
    assert (got_g[ties == 8] == 0).all()
    for i in range(len(every)):                                         # no smaller g reaches the minimum
        assert not (keys[:got_g[i], i] == keys[:, i].min()).any()


@pytest.mark.parametrize("dev", DEVICES)
def test_action_permutation_is_the_envs_own(pkg, dev):
    """legal_moves(image_g(b)) is the pi_g-permuted legal_moves(b): bit pi_g(a) of the image's mask == bit a of b's."""
    boards = np.concatenate([random_boards(4096, 2), np.stack([one_move_board(a) for a in range(4)]),
                             random_boards(512, 3) % 3])                # (small tiles: many merges)
    base = legal(pkg, dev, boards)
    assert set(1 << a for a in range(4)) <= set(base.tolist()) and len(set(base.tolist())) > 8
    for g, img in enumerate(images(boards.reshape(-1, 4, 4))):
        m = legal(pkg, dev, np.ascontiguousarray(img).reshape(-1, 16))
        for a in range(4):
            assert np.array_equal((m >> int(pi(g, a))) & 1, (base >> a) & 1), (g, a)


# ---------------------------------------------------------------------------------------------
# 2. the fused learner == a plain agent driven by the four calls on canonical boards
# ---------------------------------------------------------------------------------------------
def model_run(pkg, O, dev, env, model, steps, eps, records=None, states=None):
    """Per step: numpy canon of s, the plain agent's rows of canon(s) permuted to the env frame, the action from the
    draws (explore iff x0 < ceil(eps * 2^32), then x1 >> 30, else the first maximum), env.step, update_q_value on the
    canonical boards with the permuted action, reset(done).  The env's profile and the agent's write mode are those
    of `env` and `model`.
    `records` (a list): for every env whose step ended an episode, the record the episode log gets -- (env id,
    episode, the ENV's action, reward, max_log2, score, total return, q), q being the model's row of canon(s) read
    AFTER update_q_value and permuted to the env's frame, as four float32 bit patterns -- and, ninth, g of s.
    `states` (a list): the boards [B, 16] every step started from."""
    thr = math.ceil(eps * 4294967296.0)
    B, explored, episodes = env.num_envs, 0, 0
    for _ in range(steps):
        s = env.boards.cpu().numpy()
        if states is not None:
            states.append(s.copy())
        cs, g, _ = canon(s)
        q = env_rows(model.q_values(torch.from_numpy(cs).to(dev)).cpu().numpy(), g)
        acts = np.zeros(B, dtype=np.uint8)
        for i in range(B):
            x = O.draws(env.seed, env.env_id0 + i, env.ctr)
            if int(x[0]) < thr:
                acts[i] = int(x[1]) >> 30
                explored += 1
            else:
                acts[i] = int(np.argmax(q[i]))
        nxt, reward, done, _ = env.step(torch.from_numpy(acts).to(dev))
        cn, _, _ = canon(nxt.cpu().numpy())
        model.update_q_value(torch.from_numpy(cs).to(dev), torch.from_numpy(pi(g, acts).astype(np.uint8)).to(dev),
                             reward, torch.from_numpy(cn).to(dev), done)
        episodes += int(done.sum().item())
        if records is not None and bool(done.any()):
            over = np.flatnonzero(done.cpu().numpy())
            live = env_rows(model.q_values(torch.from_numpy(cs).to(dev)).cpu().numpy(), g).view(np.uint32)
            aux, rew, mx = env.aux_fields(), reward.cpu().numpy(), env.max_log2.cpu().numpy()   # (before the reset)
            for i in over.tolist():
                records.append((env.env_id0 + i, int(aux["episode"][i]), int(acts[i]), float(rew[i]), int(mx[i]),
                                int(aux["score"][i]), float(aux["ep_return"][i]), tuple(live[i].tolist()), int(g[i])))
        env.reset(done)
    return explored, episodes


def check_fused_equals_model(pkg, O, dev, B, independent):
    steps, eps = 160, 0.3
    # (2^18 slots: 256 envs with private rows create ~35 000 rows in 160 steps, and the key set must stay open)
    env, agent = make(pkg, dev, B, True, independent=independent, eps=eps, cap=18)
    env_m, model = make(pkg, dev, B, False, independent=independent, eps=eps, cap=18)
    for cut in (1, 63, steps - 64):                                     # (the row-cache hand-over between launches)
        agent.fused_rollout(env, cut)
    explored, episodes = model_run(pkg, O, dev, env_m, model, steps, eps)
    sync(dev)
    st = agent.stats()
    print(f"B {B} independent {independent}: rows {st['inserts']} explored {st['explored']} episodes {st['episodes']}")
    assert torch.equal(env.boards, env_m.boards), "boards differ"
    assert torch.equal(env.aux, env_m.aux), "aux records differ"
    assert rows_of(agent) == rows_of(model)
    assert st["inserts"] == model.stats()["inserts"] == agent.table_size()
    assert st["explored"] == explored and st["episodes"] == episodes and st["steps"] == B * steps
    assert st["drops"] == 0 and agent.check_status() == 0 and model.check_status() == 0
    assert episodes >= B // 8, "the span must cover the reset path"    # (one env alone may play on past 160 steps)
    assert not agent.frozen and not model.frozen
    agent.verify_table()


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [1, 77, 256])
def test_fused_learner_equals_the_model_private_rows(pkg, O, dev, B):
    check_fused_equals_model(pkg, O, dev, B, True)


@pytest.mark.parametrize("dev", DEVICES)
def test_fused_learner_equals_the_model_shared_table_one_env(pkg, O, dev):
    check_fused_equals_model(pkg, O, dev, 1, False)


# ---------------------------------------------------------------------------------------------
# 3. shared table: the exact key set under races
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_shared_table_key_set_is_the_folded_plain_one(pkg, dev):
    """epsilon = 1: the action never depends on the table, so a plain run and a folded run play the same games."""
    B, steps = 4096, 64
    env_p, plain = make(pkg, dev, B, False, cap=20, eps=1.0)
    env_s, folded = make(pkg, dev, B, True, cap=20, eps=1.0)
    plain.fused_rollout(env_p, steps)
    folded.fused_rollout(env_s, steps)
    sync(dev)
    assert torch.equal(env_p.boards, env_s.boards) and torch.equal(env_p.aux, env_s.aux)
    kp, _ = plain.export_rows()
    ks, _ = folded.export_rows()
    want = np.unique(canon(unpack(kp))[2])
    assert np.array_equal(np.sort(ks), want)
    assert folded.stats()["inserts"] == len(want) == len(ks)
    assert np.array_equal(canon(unpack(ks))[2], ks)                     # every stored key is its own canonical image
    assert folded.verify_table()["rows"] == len(want) and plain.verify_table()["rows"] == len(kp)
    assert len(ks) < len(kp)
    assert folded.check_status() == 0 and folded.stats()["drops"] == 0
    print(f"rows: plain {len(kp)} folded {len(ks)} ratio {len(kp) / len(ks):.3f} ({B} envs x {steps} steps, epsilon 1)")


# ---------------------------------------------------------------------------------------------
# 4. closed key set: line summaries, drops, checkpoint / resume with visit rows
# ---------------------------------------------------------------------------------------------
def frozen_learner(pkg, dev, line_summaries, strict_td=False):
    """Private rows, epsilon 0.3, launches of 8 until the agent's own policy closes the key set (2^14 slots at
    freeze_load 0.5) -- private rows make the run a function of its inputs, so two calls give the same learner."""
    env, agent = make(pkg, dev, 256, True, independent=True, cap=14, freeze_load=0.5, strict_td=strict_td)
    agent.line_summaries = line_summaries
    with _quiet():
        for _ in range(40):
            agent.fused_rollout(env, 8)
            if agent.frozen:
                break
    assert agent.frozen
    agent.epsilon = 0.2
    return env, agent


def same_learner(a_env, a, b_env, b):
    assert torch.equal(a_env.boards, b_env.boards) and torch.equal(a_env.aux, b_env.aux)
    assert rows_of(a) == rows_of(b)
    sa, sb = a.stats(), b.stats()
    for k in ("steps", "episodes", "valid_moves", "score_sum", "explored", "drops", "inserts"):
        assert sa[k] == sb[k], k


@pytest.mark.parametrize("dev", DEVICES)
def test_closed_key_set(pkg, dev):
    env, agent = frozen_learner(pkg, dev, True)
    env2, slotwise = frozen_learner(pkg, dev, False)
    same_learner(env, agent, env2, slotwise)
    rows = agent.table_size()
    with _quiet():
        agent.fused_rollout(env, 40)
        slotwise.fused_rollout(env2, 40)
        sd_env, sd_agent = env.state_dict(), agent.state_dict()
        agent.fused_rollout(env, 60)
        slotwise.fused_rollout(env2, 60)
    sync(dev)
    assert agent._summarised and not slotwise._summarised
    words = agent.table.view(torch.int64).reshape(-1, 4)
    assert bool((words[:, 3] != 0).any()) and not bool((slotwise.table.view(torch.int64).reshape(-1, 4)[:, 3] != 0).any())
    same_learner(env, agent, env2, slotwise)
    st = agent.stats()
    assert st["drops"] > 0 and agent.table_size() == rows and agent.check_status() == 0
    assert sd_agent["symmetric"] is True and "visit_rows" in sd_agent
    # checkpoint / resume in the middle == the uninterrupted run, visit rows included
    env3, resumed = make(pkg, dev, 256, True, independent=True, cap=14, freeze_load=0.5)
    env3.load_state_dict(sd_env)
    resumed.load_state_dict(sd_agent)
    resumed.epsilon = 0.2
    with _quiet():
        resumed.fused_rollout(env3, 60)
    sync(dev)
    assert resumed.frozen
    assert torch.equal(env.boards, env3.boards) and torch.equal(env.aux, env3.aux)
    assert rows_of(agent) == rows_of(resumed)
    s3 = resumed.stats()
    for k in ("steps", "episodes", "valid_moves", "score_sum", "explored", "drops", "inserts"):
        assert st[k] == s3[k], k
    print(f"closed key set: {rows} rows, {st['drops']} drops of {st['steps']} steps")


# ---------------------------------------------------------------------------------------------
# 5. the player
# ---------------------------------------------------------------------------------------------
def dead_board():
    return torch.tensor([1 + ((r + c) & 1) for r in range(4) for c in range(4)], dtype=torch.uint8)


def trained(pkg, dev, B=256, **kw):
    env, agent = make(pkg, dev, B, True, **kw)
    agent.fused_rollout(env, 200)
    env.boards[:3] = dead_board().to(dev)[None, :]
    return env, agent


@pytest.mark.parametrize("dev", DEVICES)
def test_player_equals_the_four_call_loop(pkg, dev):
    env, agent = trained(pkg, dev)
    loop_env = twin_of(pkg, env)
    before = agent.table.clone()
    agent.status.zero_()
    for cut in (1, 63, 96):
        agent.play_rollout(env, cut)
    evaluate = importlib.import_module("evaluate")
    args = types.SimpleNamespace(seed=loop_env.seed, epsilon=0.0, steps_per_launch=160, max_steps=loop_env.ctr + 160)
    st_loop = evaluate.play_legal_moves(torch, agent, loop_env, args, 1 << 62)
    sync(dev)
    st = agent.play_stats()
    assert torch.equal(env.boards, loop_env.boards) and torch.equal(env.aux, loop_env.aux)
    assert st["steps"] == st_loop["steps"] == 160 * 256 and st["valid_moves"] == st_loop["valid_moves"]
    assert st["episodes"] == st_loop["episodes"] >= 64 and st["max_tile_hist"] == st_loop["max_tile_hist"]
    assert st["explored"] == 0 and torch.equal(agent.table, before) and int(agent.status.item()) == 0


@pytest.mark.parametrize("dev", DEVICES)
def test_player_exploration_against_the_model(pkg, O, dev):
    """The rows the model decides on come from the numpy canonical form and a PLAIN lookup of the canonical boards,
    permuted here -- not from the folded agent's q_values."""
    model_actions = importlib.import_module("test_play_rollout").model_actions
    B, steps, eps = 256, 120, 0.3
    env, agent = trained(pkg, dev, B)
    model = twin_of(pkg, env)
    _, reader = make(pkg, dev, B, False)                                # a plain agent reading the same table
    reader.table = agent.table
    before = agent.table.clone()
    agent.play_rollout(env, 50, epsilon=eps)
    agent.play_rollout(env, steps - 50, epsilon=eps)
    explored = 0
    for _ in range(steps):
        cs, g, _ = canon(model.boards.cpu().numpy())
        q = env_rows(reader.q_values(torch.from_numpy(cs).to(dev)).cpu().numpy(), g)
        assert np.array_equal(q.view(np.uint32), agent.q_values(model.boards).cpu().numpy().view(np.uint32))
        acts, e = model_actions(O, q, model.legal_moves().cpu().numpy(), model.seed, model.env_id0, model.ctr, eps)
        explored += e
        _, _, done, _ = model.step(torch.from_numpy(acts).to(dev))
        model.reset(done)
    sync(dev)
    st = agent.play_stats()
    assert torch.equal(env.boards, model.boards) and torch.equal(env.aux, model.aux)
    assert st["explored"] == explored and 0.2 * B * steps < explored < 0.4 * B * steps
    assert st["steps"] == B * steps and st["episodes"] > 0 and torch.equal(agent.table, before)


# ---------------------------------------------------------------------------------------------
# 6. ABI and surface
# ---------------------------------------------------------------------------------------------
def test_both_libraries_export_canonicalize(pkg):
    N = pkg._native
    assert "q2048_canonicalize" in N._SIGNATURES and N.FLAG_SYMMETRIC == FLAG_SYMMETRIC
    assert hasattr(N.host_lib(), "q2048_canonicalize") and N.host_lib().q2048_abi_version() == 7
    assert hasattr(N.lib(), "q2048_canonicalize") and N.lib().q2048_abi_version() == 7 == N.ABI_VERSION
    with open(os.path.join(REPO, "include", "q2048.h")) as fh:
        text = fh.read()
    assert "int q2048_canonicalize(" in text and "#define Q2048_FLAG_SYMMETRIC (1u << 26)" in text


@pytest.mark.parametrize("which", ["hip", "host"])
def test_argument_errors_need_no_device(pkg, which):
    """Both libraries check their arguments on the host before anything runs: made-up addresses do."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    b, a, t, s, x = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    canon_ = L.q2048_canonicalize
    assert canon_(b, 8, 5, x, s, None) == -4 and canon_(b, 8, 3, x, s, None) == -4      # UNSUPPORTED
    assert canon_(b, -1, 4, x, s, None) == -2                                              # SIZE
    assert canon_(None, 8, 4, x, s, None) == -1                                            # NULL
    assert canon_(b + 8, 8, 4, x, s, None) == -3 and canon_(b, 8, 4, x + 4, s, None) == -3  # ALIGN
    assert canon_(b, 0, 4, x, s, None) == 0 and canon_(b, 0, 4, None, None, None) == 0     # B = 0: a no-op
    assert canon_(None, 0, 4, None, None, None) == -1                                      # (arguments still checked)
    S = FLAG_SYMMETRIC
    fused = lambda n, flags: L.q2048_fused_rollout(b, a, t, 12, 8, n, 1, 0.1, 0.1, 0.9, 1, 0, 0, flags, None, None, s, None)  # noqa: E731
    play = lambda n, flags: L.q2048_play_rollout(b, a, t, 12, 8, n, 1, 0.1, 1, 0, 0, flags, None, None, s, None)             # noqa: E731
    look = lambda n, flags: L.q2048_q_lookup(t, 12, b, 8, n, 0, flags, x, None, s, None)                                    # noqa: E731
    for f in (fused, play, look):
        assert f(5, S) == -4                                            # n = 5 with the flag: UNSUPPORTED
        for bit in (1 << 25, 1 << 27, 1 << 30, 1 << 31):
            assert f(4, bit) == -7 and f(4, bit | S) == -7, bit         # still refused
    opts = N.RolloutOpts()
    assert L.q2048_fused_rollout_opts(b, a, t, 12, 8, 5, 1, 0.1, 0.1, 0.9, 1, 0, 0, S, None, None, s, C.byref(opts), None) == -4
    assert L.q2048_fused_rollout_log(b, a, t, 12, 8, 5, 1, 0.1, 0.1, 0.9, 1, 0, 0, S, None, None, s, x, 4, s, None) == -4
    # the entry points that refuse the flag
    assert L.q2048_q_choose(t, 12, b, 8, 4, 0.1, 1, 0, 0, S, x, s, None) == -7
    assert L.q2048_q_choose_cached(t, 12, b, 8, 4, 0.1, 1, 0, 0, S, None, x, s, None) == -7
    assert L.q2048_q_choose_draws(t, 12, b, x, x, 8, 4, 0.1, 0, S, x, s, None) == -7
    assert L.q2048_q_update(t, 12, b, x, x, b, x, 8, 4, 0.1, 0.9, 0, S, None, s, None) == -7
    assert L.q2048_q_update_cached(t, 12, b, x, x, b, x, 8, 4, 0.1, 0.9, 0, S, None, None, s, None) == -7
    ws = 0x10000
    assert L.q2048_det_rollout(b, a, t, 12, 8, 4, 1, 0.1, 0.1, 0.9, 1, 0, 0, S, None, None, s, ws, 1 << 20, None) == -7
    assert L.q2048_det_rollout_cached(b, a, t, 12, 8, 4, 1, 0.1, 0.1, 0.9, 1, 0, 0, S, None, None, s, ws, 1 << 20, None, None) == -7
    assert L.q2048_env_reset_ex(b, a, None, 8, 4, 1, 0, S, None) == -7
    assert L.q2048_env_step_ex(b, a, x, 8, 4, 1, 0, 0, S, None, x, x, x, s, None) == -7


@pytest.mark.parametrize("dev", DEVICES)
def test_flag_with_play_only_is_inert_and_n5_is_refused(pkg, dev):
    N = pkg._native
    env, agent = make(pkg, dev, 64, True, cap=12, eps=1.0)
    ref_env, ref = make(pkg, dev, 64, False, cap=12, eps=1.0)
    agent.fused_rollout(env, 20, play_only=True)                        # SYMMETRIC | PLAY_ONLY
    ref.fused_rollout(ref_env, 20, play_only=True)
    sync(dev)
    assert torch.equal(env.boards, ref_env.boards) and torch.equal(env.aux, ref_env.aux) and agent.table_size() == 0
    with pytest.raises(ValueError):
        pkg.BatchedQLearningAgent(10, capacity_log2=12, device=dev, board_size=5, placement="plain", symmetric=True)
    env5 = pkg.BatchedGame2048Env(8, 5, dev, 1, 0)
    a5 = pkg.BatchedQLearningAgent(10, capacity_log2=12, device=dev, board_size=5, placement="plain", seed=1)
    a5._sym = N.FLAG_SYMMETRIC                                          # the flag forced past the constructor
    with pytest.raises(N.NativeError) as err:
        a5.fused_rollout(env5, 1)
    assert err.value.code == -4
    with pytest.raises(N.NativeError) as err:
        a5.q_values(env5.boards)
    assert err.value.code == -4


def test_python_surface(pkg, tmp_path):
    env, agent = make(pkg, "cpu", 32, True, cap=12)
    plain_env, plain = make(pkg, "cpu", 32, False, cap=12)
    assert agent.symmetric is True and plain.symmetric is False
    for call in (lambda: agent.choose_action(env.boards),
                 lambda: agent.update_q_value(env.boards, torch.zeros(32, dtype=torch.uint8), torch.zeros(32),
                                              env.boards, torch.zeros(32, dtype=torch.uint8)),
                 lambda: agent.deterministic_rollout(env, 1)):
        with pytest.raises(ValueError, match="Q2048_FLAG_SYMMETRIC"):
            call()
    agent.fused_rollout(env, 40)
    plain.fused_rollout(plain_env, 40)
    sd, sd_plain = agent.state_dict(), plain.state_dict()
    assert sd["symmetric"] is True and "symmetric" not in sd_plain
    _, other = make(pkg, "cpu", 32, True, cap=12)
    _, other_plain = make(pkg, "cpu", 32, False, cap=12)
    with pytest.raises(ValueError, match="folded"):
        other_plain.load_state_dict(sd)
    with pytest.raises(ValueError, match="folded"):
        other.load_state_dict(sd_plain)
    other.load_state_dict(sd)
    other_plain.load_state_dict(sd_plain)                               # a checkpoint without the field is plain
    assert rows_of(other) == rows_of(agent) and rows_of(other_plain) == rows_of(plain)
    with pytest.raises(ValueError, match="folded"):
        plain.merge_from(agent)
    with pytest.raises(ValueError, match="folded"):
        agent.merge_from(plain)
    assert other.merge_from(agent, mode="maxabs")["read"] == agent.table_size()
    # q_values: env-frame rows; export_dict: canonical states only
    boards = env.boards.cpu().numpy()
    cs, g, _ = canon(boards)
    _, reader = make(pkg, "cpu", 32, False, cap=12)
    reader.table = agent.table
    want = env_rows(reader.q_values(torch.from_numpy(cs)).numpy(), g)
    assert np.array_equal(agent.q_values(env.boards).numpy().view(np.uint32), want.view(np.uint32))
    cb, cg = agent.canonicalize(env.boards)
    assert np.array_equal(cb.numpy(), cs) and np.array_equal(cg.numpy(), g)
    d = agent.export_dict()
    assert len(d) == agent.table_size() > 0
    for state in d:
        raw = np.array(state)
        log2 = np.where(raw > 0, np.log2(np.maximum(raw, 1)), 0).astype(np.uint8).reshape(1, 16)
        assert np.array_equal(canon(log2)[0], log2)
    # merge_tables.py refuses to mix the two kinds
    torch.save(sd, tmp_path / "folded.pt")
    torch.save(sd_plain, tmp_path / "plain.pt")
    run = lambda *a: subprocess.run([sys.executable, os.path.join(REPO, "merge_tables.py"), *a],   # noqa: E731
                                    capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    help_ = run("--help")
    assert help_.returncode == 0
    mixed = run("folded.pt", "plain.pt", "--out", "m.pt", "--device", "cpu")
    assert mixed.returncode != 0 and "cannot be merged" in mixed.stderr
    both = run("folded.pt", "folded.pt", "--out", "m.pt", "--device", "cpu")
    assert both.returncode == 0, both.stderr[-2000:]
    assert torch.load(tmp_path / "m.pt", map_location="cpu", weights_only=False)["symmetric"] is True


def test_train_and_evaluate_scripts_agree_on_symmetric(pkg, tmp_path):
    py = lambda script, *a: subprocess.run([sys.executable, os.path.join(REPO, script), "--device", "cpu", *a],   # noqa: E731
                                           capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    p = py("train.py", "--symmetric", "--num-envs", "64", "--episodes", "3", "--capacity-log2", "16", "--save", "q.pt",
           "--eval-every", "1", "--eval-envs", "64")
    assert p.returncode == 0, p.stderr[-2000:]
    sd = torch.load(tmp_path / "q.pt", map_location="cpu", weights_only=False)
    assert sd["symmetric"] is True and len(sd["q"]) > 0
    assert np.array_equal(canon(unpack(sd["keys"]))[2], sd["keys"])     # the saved table is folded
    assert len(open(tmp_path / "eval_log.jsonl").read().splitlines()) == 3
    common = ("evaluate.py", "--model", "q.pt", "--num-envs", "64", "--episodes", "1", "--steps-per-launch", "32")
    fused, loop = py(*common, "--fused"), py(*common)
    assert fused.returncode == 0, fused.stderr[-2000:]
    assert loop.returncode == 0, loop.stderr[-2000:]
    a, b = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (loop, fused))
    assert a["symmetric"] is True and b["symmetric"] is True and b["fused"] is True
    for key in ("games", "env_steps", "mean_score", "max_tile_hist", "valid_move_frac"):
        assert a[key] == b[key], key
    for bad in (("--board-size", "5"), ("--agent", "row-tuple"), ("--deterministic",)):
        r = py("train.py", "--symmetric", "--num-envs", "64", "--episodes", "1", *bad)
        assert r.returncode != 0 and "--symmetric" in r.stderr, bad
