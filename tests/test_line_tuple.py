"""The line-tuple learner (rows AND columns as features, W = float32 [8, 65536, 4]): the five entry points q2048_lt_choose,
q2048_lt_lookup, q2048_lt_update, q2048_lt_fused_rollout and q2048_lt_play_rollout against a numpy model, and
BatchedLineTupleAgent's checkpoint and promotion.  (The scripts: test_line_tuple_scripts.py.)

Which test executes which kernel (device) / function (CPU twin):
  k_lt_lookup         test_lookup_at_the_edges, test_lookup_reads_each_feature_from_its_own_table, test_65536_boards
  k_lt_choose         test_choose_at_the_edges (greedy incl. exact ties; epsilon = 0.3 against the oracle's draws), test_65536_boards
  k_lt_update         test_update_on_entries_that_cannot_race
  k_lt_fused_rollout  test_fused_rollout_with_frozen_weights, test_fused_rollout_one_lane_many_steps (the carried-entry rule,
                      per feature), test_fused_rollout_one_learning_step (lt_scatter inside the fused loop)
  k_eval_play_rollout<LtEvalOf, E>   test_player_equals_the_four_call_loop, test_player_exploration_against_a_model
  the argument checks test_abi, test_argument_errors_need_no_device

The model (model_idx, model_q, model_update) is plain numpy and shares no code with csrc/; there is no oracle for this
learner.  Every comparison is exact: integers, bytes, and float32 values as bit patterns.  There is no tolerance: Q is a
fixed chain of float32 additions, ((e0+e1)+(e2+e3)) + ((e4+e5)+(e6+e7)), the TD step one float64 expression rounded
once, and a contraction of reward + (gamma * max) * mask into an fma cannot change it because the mask is 0.0 or 1.0
(the argument of test_row_tuple_kernels.py).  Helpers that are not the model come from the row-tuple test modules.
Every case runs on the CPU twin ("cpu") and on the GPU."""
import os

import numpy as np
import pytest
import torch

import test_row_tuple_kernels as K
import test_row_tuple_player as P

REPO = P.REPO
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
EDGES = [1, 63, 64, 65, 255, 256, 257, 1000]     # ends of a wave and of the 256-lane block, a partial second block, four blocks
ROOM, Q_CANARY, A_CANARY, BAD_ACTION = K.ROOM, K.Q_CANARY, K.A_CANARY, K.BAD_ACTION
ERR_NULL, ERR_SIZE, ERR_ALIGN, ERR_RANGE, ERR_FLAGS = -1, -2, -3, -6, -7
F32 = np.float32
NAMES = ("q2048_lt_choose", "q2048_lt_lookup", "q2048_lt_update", "q2048_lt_fused_rollout", "q2048_lt_play_rollout")
lib, t8, t32, bits, assert_same_bits = K.lib, K.t8, K.t32, K.bits, K.assert_same_bits


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def model_idx(boards):
    """f < 4: idx_f = sum_k (cell[4f+k] & 15) << 4k (row f);  f >= 4: idx_f = sum_k (cell[4k+(f-4)] & 15) << 4k (column
    f-4, from the top)  -> int64 [B, 8]"""
    c = (np.asarray(boards, dtype=np.int64) & 15).reshape(-1, 4, 4)            # [B, row, column]
    rows = c[:, :, 0] | (c[:, :, 1] << 4) | (c[:, :, 2] << 8) | (c[:, :, 3] << 12)
    cols = c[:, 0, :] | (c[:, 1, :] << 4) | (c[:, 2, :] << 8) | (c[:, 3, :] << 12)
    return np.concatenate([rows, cols], axis=1)


def model_q(W, boards):
    """Q(s,a) = ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7)), e_f = W[f, idx_f, a], in float32 -> float32 [B, 4]"""
    idx = model_idx(boards)
    e = [W[f, idx[:, f]] for f in range(8)]
    assert all(x.dtype == F32 for x in e)
    return ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]))


def model_update(W, s, actions, reward, s2, done, lr, gamma, inplace=False):
    """The TD step, lane after lane on one array.  -> (weights afterwards, status word)"""
    W, status = (W if inplace else W.copy()), 0
    idx_s = model_idx(s)
    for i in range(len(s)):
        a = int(actions[i])
        if a > 3:
            status |= BAD_ACTION
            continue
        max_next = float(model_q(W, s2[i:i + 1])[0].max())
        q_sa = float(model_q(W, s[i:i + 1])[0, a])
        target = float(reward[i]) + gamma * max_next * (0.0 if done[i] else 1.0)     # float64
        d = F32((lr * 0.125) * (target - q_sa))                                      # rounded once
        for f in range(8):
            W[f, idx_s[i, f], a] = F32(W[f, idx_s[i, f], a] + d)
    return W, status


def latin_boards(rng, B):
    """Lane i: four base-12 digits d0..d3 of an element of a permutation of 12^4, cell(r, c) = d[(r + c) mod 4].  Every
    row and every column holds all four digits in a fixed cyclic order, so each of the eight indices is injective in i."""
    p = rng.permutation(12 ** 4)[:B]
    d = np.stack([(p // 12 ** k) % 12 for k in range(4)], axis=1)                      # [B, 4]
    boards = np.stack([d[:, (r + c) % 4] for r in range(4) for c in range(4)], axis=1).astype(np.uint8)
    idx = model_idx(boards)
    assert boards.max() <= 11 and all(len(np.unique(idx[:, f])) == B for f in range(8)), "the construction is not injective"
    return boards


# ---------------------------------------------------------------------------------------------------------------
# the entry points, through ctypes alone
# ---------------------------------------------------------------------------------------------------------------
def lt_lookup(L, dev, weights, boards):
    B = len(boards)
    out = torch.full((B + ROOM, 4), Q_CANARY - (1 << 32), dtype=torch.int32, device=dev)
    tb = t8(dev, boards)
    assert L.q2048_lt_lookup(weights.data_ptr(), tb.data_ptr(), B, out.data_ptr(), None) == 0
    out = out.cpu().numpy().view(np.uint32)
    return out[:B], out[B:]


def lt_choose(L, dev, weights, boards, eps, seed=0, env_id0=0, ctr=0):
    B = len(boards)
    out = torch.full((B + ROOM,), A_CANARY, dtype=torch.uint8, device=dev)
    tb = t8(dev, boards)
    assert L.q2048_lt_choose(weights.data_ptr(), tb.data_ptr(), B, float(eps), seed, env_id0, ctr, out.data_ptr(),
                             None) == 0
    out = out.cpu().numpy()
    return out[:B], out[B:]


_SHARED = {}


def base_weights():
    """Random normal float32 [8, 65536, 4], built once; nobody writes it."""
    if "w" not in _SHARED:
        w = np.random.default_rng(21).standard_normal((8, 65536, 4)).astype(F32)
        w.setflags(write=False)
        _SHARED["w"] = w
    return _SHARED["w"]


def make_agent(pkg, dev, eps=0.3, lr=0.1, gamma=0.95, seed=P.SEED, id0=P.ID0, epochs=100):
    return pkg.BatchedLineTupleAgent(epochs, learning_rate=lr, discount_factor=gamma, exploration_rate=eps, seed=seed,
                                     env_id0=id0, device=dev)


# ---------------------------------------------------------------------------------------------------------------
# 1. ABI
# ---------------------------------------------------------------------------------------------------------------
def test_abi(pkg):
    N = pkg._native
    with open(os.path.join(REPO, "include", "q2048.h")) as fh:
        header = fh.read()
    for name in NAMES:
        assert name in N._SIGNATURES, name
        assert hasattr(N.host_lib(), name) and hasattr(N.lib(), name), name
        assert f"int {name}(" in header, name
    assert N.host_lib().q2048_abi_version() == 7 == N.lib().q2048_abi_version() == N.ABI_VERSION
    assert "#define Q2048_ABI_VERSION 7 " in header
    assert pkg.BatchedLineTupleAgent is __import__("q2048_amd").BatchedLineTupleAgent


@pytest.mark.parametrize("which", ["hip", "host"])
def test_argument_errors_need_no_device(pkg, which):
    """The documented order -- B, (flags,) NULL, alignment, (steps,) the scalars -- on both libraries, with made-up
    aligned addresses: every refused call also carries the errors that come later in the order, and nothing behind
    the addresses is touched (B == 0 and steps == 0 are no-ops)."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    nan, big = float("nan"), (2 ** 31 - 1) * 256 + 1
    a = [0x1000 * (k + 1) for k in range(8)]
    # (function, good arguments, required pointers, 16-byte aligned pointers, position of B, {scalar position: refused})
    entry_points = {
        "lt_choose": (L.q2048_lt_choose, [a[0], a[1], 64, 0.3, 7, 50, 3, a[2], None], (0, 1, 7), (0, 1), 2,
                      {3: (-0.1, 1.5, nan)}),
        "lt_lookup": (L.q2048_lt_lookup, [a[0], a[1], 64, a[2], None], (0, 1, 3), (0, 1, 3), 2, {}),
        "lt_update": (L.q2048_lt_update, [a[0], a[1], a[2], a[3], a[4], a[5], 64, 0.1, 0.97, a[6], None],
                      (0, 1, 2, 3, 4, 5, 9), (0, 1, 4), 6, {7: (nan,), 8: (nan,)}),
        "lt_fused_rollout": (L.q2048_lt_fused_rollout, [a[0], a[1], a[2], 64, 2, 0.3, 0.1, 0.97, 3, 50, 0, None, None,
                                                        a[3], None],
                             (0, 1, 2, 13), (0, 1, 2), 3, {5: (-0.1, 1.5, nan), 6: (nan,), 7: (nan,)}),
    }
    for name, (fn, good, pointers, aligned, b_pos, scalars) in entry_points.items():
        def call(**kw):
            args = list(good)
            for pos, value in kw.items():
                args[int(pos[1:])] = value
            return fn(*args)

        bad_scalar = {f"p{pos}": values[-1] for pos, values in scalars.items()}
        bad_align = {f"p{pos}": good[pos] + 8 for pos in aligned}
        for value in (-1, big):                                         # B before everything
            assert call(**{f"p{b_pos}": value, f"p{pointers[0]}": None}, **bad_scalar) == ERR_SIZE, name
        for pos in pointers:                                            # NULL before the alignment and the scalars
            kw = {**bad_align, **bad_scalar, f"p{pos}": None}
            assert call(**kw) == ERR_NULL, f"{name}: NULL in position {pos}"
        for pos in aligned:                                             # the alignment before the scalars
            assert call(**{f"p{pos}": good[pos] + 8}, **bad_scalar) == ERR_ALIGN, f"{name}: position {pos} off by 8 bytes"
        for pos, values in scalars.items():
            for value in values:
                assert call(**{f"p{pos}": value}) == ERR_RANGE, f"{name}: {value} in position {pos}"
        assert call(**{f"p{b_pos}": 0}) == 0, f"{name}: B = 0"
        assert call(**{f"p{b_pos}": 0, f"p{pointers[0]}": None}) == ERR_NULL, f"{name}: B = 0 is checked first"
    fn, good = entry_points["lt_fused_rollout"][:2]
    for steps, eps, code in ((-1, nan, ERR_SIZE), ((1 << 30) + 1, nan, ERR_SIZE), (0, 0.3, 0), (0, nan, ERR_RANGE)):
        args = list(good)
        args[4], args[5] = steps, eps                                   # steps before epsilon
        assert fn(*args) == code, f"lt_fused_rollout: steps = {steps}"
    # the player: the order and the flags of q2048_rt_play_rollout
    ok = P.argument_errors(L.q2048_lt_play_rollout, 0x1000, 0x2000, 0x3000, 0x4000)
    for bit in (N.FLAG_INDEPENDENT, N.FLAG_SYMMETRIC, N.FLAG_SINGLE_ENV, N.FLAG_TD_CAS, N.FLAG_PLAY_ONLY, N.FLAG_NO_LEARN,
                N.FLAG_NO_NEW_ROWS, N.FLAG_LINE_SUMMARY, 1 << 8, 1 << 23, 1 << 30, 1 << 31):
        assert ok(flags=bit) == ERR_FLAGS and ok(flags=bit | N.FLAG_ENV_DQN | N.FLAG_RESET_SHAPING) == ERR_FLAGS, bit
    assert ok(B=0) == 0 and ok(steps=0) == 0
    assert ok(B=0, boards=None) == ERR_NULL and ok(steps=0, weights=0x3008) == ERR_ALIGN
    assert ok(B=0, flags=N.FLAG_INDEPENDENT) == ERR_FLAGS


# ---------------------------------------------------------------------------------------------------------------
# 2. lt_lookup at the edges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
def test_lookup_at_the_edges(pkg, dev, B):
    """Random weights over all 8 MiB, random cells 0..31: a cell of 16..31 reads the entries of its low nibble (the
    model: & 15).  The 64 records beyond B keep their canary; the weights are not written."""
    L, W = lib(pkg, dev), base_weights()
    boards = np.random.default_rng(100 + B).integers(0, 32, size=(B, 16), dtype=np.uint8)
    boards[0, 6] = 16 + 5
    want = model_q(W, boards)
    assert_same_bits(want, model_q(W, boards & 15), "the model's own mask")
    other = boards[:1].copy()
    other[0, 6] = 4
    assert (bits(model_q(W, other)) != bits(want[:1])).any(), "cell 6 of lane 0 does not show in its row"
    weights = t32(dev, W)
    got, tail = lt_lookup(L, dev, weights, boards)
    assert_same_bits(got.view(F32), want, f"B = {B}")
    assert (tail == np.uint32(Q_CANARY)).all(), "rows written beyond B"
    assert_same_bits(weights, W, "a lookup wrote the weights")


@pytest.mark.parametrize("dev", DEVICES)
def test_lookup_reads_each_feature_from_its_own_table(pkg, dev):
    """For each f the weights are non-zero in table f only, and no board equals its transpose: a kernel that reads a
    column index from a row table, or column c as column 3 - c, or a column from the bottom, returns another row."""
    L, B = lib(pkg, dev), 257
    boards = np.random.default_rng(150).integers(0, 16, size=(B, 16), dtype=np.uint8)
    g = boards.reshape(B, 4, 4)
    assert (g != g.transpose(0, 2, 1)).any(axis=(1, 2)).all() and (g != g[:, :, ::-1]).any(axis=(1, 2)).all()
    idx = model_idx(boards)
    for f in range(8):
        W = np.zeros((8, 65536, 4), dtype=F32)
        W[f] = base_weights()[f]
        want = model_q(W, boards)
        assert_same_bits(want, (W[f, idx[:, f]] + F32(0.0)), "the model: one table")
        wrong = [model_q(W, x.reshape(B, 16)) for x in (g.transpose(0, 2, 1), g[:, :, ::-1], g[:, ::-1, :])]
        assert all((bits(w) != bits(want)).any(axis=1).mean() > 0.9 for w in wrong), f"feature {f} does not tell the images apart"
        got, _ = lt_lookup(L, dev, t32(dev, W), boards)
        assert_same_bits(got.view(F32), want, f"feature {f}")


# ---------------------------------------------------------------------------------------------------------------
# 3. lt_choose at the edges
# ---------------------------------------------------------------------------------------------------------------
def weights_with_ties(B, boards):
    """base_weights() with hand-set entries: on lane 0 all eight entries zero (four actions tie: action 0), and on up to
    five more lanes seven entries zero and one -- of feature k mod 8, so rows and columns both carry one -- a row of
    K.TIES, whose maximum two actions share.  -> (weights, the tied lanes, the action each must get)"""
    W = base_weights().copy()
    idx = model_idx(boards)
    lanes = [0] + sorted({i for i in (1, 62, 63, 64, B - 1) if 0 < i < B})
    rows = [K.TIES[3]] + [K.TIES[k % 3] for k in range(len(lanes) - 1)]
    for lane in lanes:
        for f in range(8):
            W[f, idx[lane, f]] = 0.0
    for k, (lane, row) in enumerate(zip(lanes, rows)):
        W[(3 * k) % 8, idx[lane, (3 * k) % 8]] = row
    first = [int(np.argmax(np.asarray(row, dtype=F32))) for row in rows]
    q = model_q(W, boards[lanes])      # two special lanes could share an entry: what the lanes read is checked, not assumed
    for k, row in enumerate(rows):
        assert np.array_equal(q[k], np.asarray(row, dtype=F32)), f"lane {lanes[k]} does not read its hand-set row"
    return W, lanes, first


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
def test_choose_at_the_edges(pkg, O, dev, B):
    """epsilon = 0: the model's argmax (the first maximum wins), on lanes where two and where four actions tie exactly.
    epsilon = 0.3 with (seed, env_id0, ctr) = (7, 2^33 + 5, 3): lane i explores when draw_uniform(x0) < epsilon and then
    takes draw_action(x1), x = the oracle's draws of env env_id0 + i (B >= 63: both branches occur, see the row-tuple
    test)."""
    L = lib(pkg, dev)
    boards = K.random_boards(np.random.default_rng(200 + B), B)
    W, lanes, first = weights_with_ties(B, boards)
    weights = t32(dev, W)
    greedy = np.argmax(model_q(W, boards), axis=1).astype(np.uint8)
    assert greedy[lanes].tolist() == first
    if B > 1:
        assert any(a > 0 for a in first), "no tie between two non-first actions"
    got, tail = lt_choose(L, dev, weights, boards, 0.0)
    assert np.array_equal(got, greedy), f"greedy actions differ on lanes {np.flatnonzero(got != greedy)[:8].tolist()}"
    assert (tail == A_CANARY).all(), "actions written beyond B"

    eps, seed, id0, ctr = 0.3, 7, (1 << 33) + 5, 3
    x = np.stack([O.draws(seed, id0 + i, ctr) for i in range(B)])
    explore = np.array([O.draw_uniform(v) < eps for v in x[:, 0]])
    want = np.where(explore, [O.draw_action(v) for v in x[:, 1]], greedy).astype(np.uint8)
    if B >= 63:
        assert explore.any() and not explore.all()
        assert (want[~explore] != 0).any(), "every greedy lane takes what zero weights would give"
    got, tail = lt_choose(L, dev, weights, boards, eps, seed, id0, ctr)
    assert np.array_equal(got, want), f"actions differ on lanes {np.flatnonzero(got != want)[:8].tolist()}"
    assert (tail == A_CANARY).all(), "actions written beyond B"
    assert_same_bits(weights, W, "choosing wrote the weights")


@pytest.mark.parametrize("dev", DEVICES)
def test_65536_boards(pkg, O, dev):
    """256 full blocks of mid-game boards (hot entries shared by most of the batch, as in a rollout): rows bit for bit,
    greedy actions equal, and the read-only pass leaves W bit-identical."""
    L, W = lib(pkg, dev), base_weights()
    boards, _ = K.midgame_boards(O)
    want = model_q(W, boards)
    weights = t32(dev, W)
    got, tail = lt_lookup(L, dev, weights, boards)
    assert_same_bits(got.view(F32), want, "65,536 boards")
    assert (tail == np.uint32(Q_CANARY)).all(), "rows written beyond B"
    greedy = np.argmax(want, axis=1).astype(np.uint8)
    assert np.bincount(greedy, minlength=4).min() > 0
    got, tail = lt_choose(L, dev, weights, boards, 0.0, 41, 0, 40)
    assert np.array_equal(got, greedy), f"{int((got != greedy).sum())} greedy actions differ"
    assert (tail == A_CANARY).all(), "actions written beyond B"
    assert_same_bits(weights, W, "a read-only pass wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 4. lt_update on entries that cannot race
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
def test_update_on_entries_that_cannot_race(pkg, dev, B):
    """s: `latin_boards` (cells 0..11, each of the eight indices distinct across lanes); s': cells 12..15 only.  No lane
    reads an entry another lane writes (asserted on the inputs), so the result does not depend on the order of the
    lanes and the sequential model is the specification.  All 8 MiB are compared: exactly 8 values per good lane moved.
    One lane carries action 7 (B > 2): it writes nothing and sets Q2048_STATUS_BAD_ACTION."""
    L, W = lib(pkg, dev), base_weights()
    rng = np.random.default_rng(300 + B)
    s = latin_boards(rng, B)
    s2 = rng.integers(12, 16, size=(B, 16), dtype=np.uint8)
    idx, idx2 = model_idx(s), model_idx(s2)
    for f in range(8):
        assert len(np.unique(idx[:, f])) == B and not np.intersect1d(idx[:, f], idx2[:, f]).size, f"feature {f} can race"
    actions = rng.integers(0, 4, size=B, dtype=np.uint8)
    bad = B // 2 if B > 2 else None
    if bad is not None:
        actions[bad] = 7
    reward = rng.standard_normal(B).astype(F32)
    done = (rng.random(B) < 0.3).astype(np.uint8)
    lr, gamma = 0.1, 0.97
    want, want_status = model_update(W, s, actions, reward, s2, done, lr, gamma)
    good = B - (bad is not None)
    assert want_status == (BAD_ACTION if bad is not None else 0)
    assert int((bits(want) != bits(W)).sum()) == 8 * good

    weights, status = t32(dev, W), torch.zeros(1, dtype=torch.int32, device=dev)
    ts, ts2, ta, tr, td = t8(dev, s), t8(dev, s2), t8(dev, actions), t32(dev, reward), t8(dev, done)
    assert L.q2048_lt_update(weights.data_ptr(), ts.data_ptr(), ta.data_ptr(), tr.data_ptr(), ts2.data_ptr(),
                             td.data_ptr(), B, lr, gamma, status.data_ptr(), None) == 0
    got = weights.cpu().numpy()
    assert int(status.item()) == want_status
    assert_same_bits(got, want, f"B = {B}")
    assert int((bits(got) != bits(W)).sum()) == 8 * good
    for t, a in ((ts, s), (ts2, s2), (ta, actions), (td, done)):
        assert np.array_equal(t.cpu().numpy(), a), "an input was written"
    assert_same_bits(tr, reward, "the rewards were written")


# ---------------------------------------------------------------------------------------------------------------
# 5.-7. the fused learner against the four-call loop of the same agent class
# ---------------------------------------------------------------------------------------------------------------
def fused_run(pkg, dev, W, B, launches, seed, id0, eps, lr, gamma, boards=None):
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    agent = make_agent(pkg, dev, eps, lr, gamma, seed, id0)
    agent.weights.copy_(torch.from_numpy(W))
    if boards is not None:
        env.boards.copy_(torch.from_numpy(boards))
    for k in launches:
        agent.fused_rollout(env, k)
    assert agent.check_status() == 0
    return env, agent


def four_call_run(pkg, O, dev, W, B, steps, seed, id0, eps, lr, gamma, boards=None, learn=False):
    """choose_action -> env.step -> (model_update on W, mirrored into the agent) -> env.reset(done), `steps` times: the
    loop the fused learner replaces, on entry points tests 2-3 have pinned to the model.  -> (env, W afterwards, the
    statistics the fused learner counts, the transitions)"""
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    agent = make_agent(pkg, dev, eps, lr, gamma, seed, id0)
    W = W.copy()
    agent.weights.copy_(torch.from_numpy(W))
    if boards is not None:
        env.boards.copy_(torch.from_numpy(boards))
    st = {"steps": 0, "episodes": 0, "valid_moves": 0, "explored": 0, "score_sum": 0}
    trans = []
    for t in range(steps):
        s = env.boards.cpu().numpy().copy()
        actions = agent.choose_action(env.boards)
        s2, reward, done, _ = env.step(actions)
        s2, a, r, d = s2.cpu().numpy().copy(), actions.cpu().numpy(), reward.cpu().numpy().copy(), done.cpu().numpy().copy()
        st["steps"] += B
        st["episodes"] += int(d.sum())
        st["valid_moves"] += int((s != s2).any(axis=1).sum())            # a move that changes the board, spawn included
        st["score_sum"] += int(env.score.cpu().numpy()[d].sum())
        if eps > 0.0:
            st["explored"] += sum(O.draw_uniform(O.draws(seed, id0 + i, t)[0]) < eps for i in range(B))
        if learn:
            before = W[np.arange(8)[None, :], model_idx(s), a[:, None]].copy()
            model_update(W, s, a, r, s2, d, lr, gamma, inplace=True)
            if B > 1:
                agent.weights.copy_(torch.from_numpy(W))
            else:
                mirror(agent, W, s, a)
            trans.append((s, a, s2, d, before))
        env.reset(done)
    return env, W, st, trans


def mirror(agent, W, s, a):
    """The eight values model_update wrote for one lane, into the agent's weights."""
    f, idx = torch.arange(8), torch.from_numpy(model_idx(s)[0])
    agent.weights[f, idx, int(a[0])] = torch.from_numpy(W[np.arange(8), model_idx(s)[0], int(a[0])]).to(agent.weights.device)


def assert_same_run(env, agent, env_loop, st_loop, what):
    assert torch.equal(env.boards.cpu(), env_loop.boards.cpu()), \
        f"{what}: boards differ on {int((env.boards.cpu() != env_loop.boards.cpu()).any(dim=1).sum())} lanes"
    assert torch.equal(env.aux.cpu(), env_loop.aux.cpu()), f"{what}: aux records differ"
    st = agent.stats()
    for key, want in st_loop.items():
        assert st[key] == want, f"{what}: {key} {st[key]} != {want}"
    return st


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B,steps,eps", [(257, 100, 0.3), (1000, 120, 0.0)])
def test_fused_rollout_with_frozen_weights(pkg, O, dev, B, steps, eps):
    """learning_rate = 0: every lane is a function of W alone, so the four-call loop is the specification at any batch
    size.  Launches of 1 and steps - 1 steps: the entries carried from step to step, the entries gathered again after
    a reset and the first gather of a launch all decide actions here.  Boards, aux records and statistics equal the
    loop's; the weights are bit for bit what was loaded.  Teeth: on zero weights the same run ends on other boards in
    more than half of the lanes (CPU twin: 257 of 257 and 1000 of 1000)."""
    seed, id0, gamma = 17, 1000, 0.97
    W = (0.5 * np.random.default_rng(500 + B).standard_normal((8, 65536, 4))).astype(F32)
    env_loop, _, st_loop, _ = four_call_run(pkg, O, dev, W, B, steps, seed, id0, eps, 0.0, gamma)
    env, agent = fused_run(pkg, dev, W, B, (1, steps - 1), seed, id0, eps, 0.0, gamma)
    st = assert_same_run(env, agent, env_loop, st_loop, f"B = {B}")
    assert st["episodes"] > 0 and (st["explored"] == 0) == (eps == 0.0)
    assert_same_bits(agent.weights, W, "frozen weights were written")
    env0, _ = fused_run(pkg, dev, np.zeros_like(W), B, (1, steps - 1), seed, id0, eps, 0.0, gamma)
    differ = int((env0.boards.cpu() != env.boards.cpu()).any(dim=1).sum())
    print(f"zero weights end on other boards in {differ} of {B} lanes")
    assert differ > B // 2, f"the weights decide the boards of only {differ} of {B} lanes"


@pytest.mark.parametrize("dev", DEVICES)
def test_fused_rollout_one_lane_many_steps(pkg, O, dev):
    """THE CARRIED-ENTRY RULE.  B = 1, lr 0.1, gamma 0.97, epsilon 0.3, 300 steps in launches of 1, 63 and 236: one lane
    is the sequential learner, so the expected weights are model_update applied step by step to the transitions of the
    four-call loop (the draws make them the same transitions).  All 8 MiB bit for bit, boards and aux equal.  The fused
    kernel gathers s' BEFORE it writes s and carries those entries into the next step: per feature, an entry whose
    index did not change takes gathered + d -- the test counts, from the model, the steps in which s and s' share an
    index at a row feature and at a column feature without done, and needs both (seed 5: see the print)."""
    seed, id0, eps, lr, gamma, cuts = 5, 77, 0.3, 0.1, 0.97, (1, 63, 236)
    W = (0.5 * np.random.default_rng(700).standard_normal((8, 65536, 4))).astype(F32)
    env_loop, want, st_loop, trans = four_call_run(pkg, O, dev, W, 1, sum(cuts), seed, id0, eps, lr, gamma, learn=True)
    shared = np.array([(model_idx(s)[0] == model_idx(s2)[0]) & (not d[0]) for s, _, s2, d, _ in trans])    # [steps, 8]
    moved = np.array([(s != s2).any() for s, _, s2, _, _ in trans])
    rows, cols = int(shared[:, :4].any(axis=1).sum()), int(shared[:, 4:].any(axis=1).sum())
    print(f"steps that carry a written entry: {rows} at a row feature, {cols} at a column feature "
          f"({int((shared.any(axis=1) & moved).sum())} of them on a move that changed the board); "
          f"episodes {st_loop['episodes']}")
    assert rows > 0 and cols > 0 and (shared[:, :4].any(axis=1) & moved).any() and (shared[:, 4:].any(axis=1) & moved).any()
    env, agent = fused_run(pkg, dev, W, 1, cuts, seed, id0, eps, lr, gamma)
    assert_same_run(env, agent, env_loop, st_loop, "B = 1")
    assert_same_bits(agent.weights, want, "300 sequential steps")
    assert (bits(want) != bits(W)).sum() > 300


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [65, 257, 1000])
def test_fused_rollout_one_learning_step(pkg, O, dev, B):
    """One step with gamma = 0, lr = 0.1, epsilon = 0.3 from `latin_boards`: with gamma = 0 the step does not read s',
    and the entries of s are private to the lane, so model_update on the actions and rewards of the four-call loop is
    the specification.  All weights bit for bit, exactly 8 B values changed; boards, aux and statistics equal."""
    seed, id0, eps, lr, gamma = 23, 4000, 0.3, 0.1, 0.0
    rng = np.random.default_rng(600 + B)
    W = (0.5 * rng.standard_normal((8, 65536, 4))).astype(F32)
    boards = latin_boards(rng, B)
    env_loop, want, st_loop, _ = four_call_run(pkg, O, dev, W, B, 1, seed, id0, eps, lr, gamma, boards=boards, learn=True)
    assert int((bits(want) != bits(W)).sum()) == 8 * B and 0 < st_loop["explored"] < B
    env, agent = fused_run(pkg, dev, W, B, (1,), seed, id0, eps, lr, gamma, boards=boards)
    assert_same_run(env, agent, env_loop, st_loop, f"B = {B}")
    got = agent.weights.cpu().numpy()
    assert_same_bits(got, want, f"B = {B}")
    assert int((bits(got) != bits(W)).sum()) == 8 * B


# ---------------------------------------------------------------------------------------------------------------
# 8. the player
# ---------------------------------------------------------------------------------------------------------------
def random_agent(pkg, dev, **kw):
    agent = make_agent(pkg, dev, **kw)
    agent.weights.copy_(torch.from_numpy(base_weights().copy()))
    return agent


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
@pytest.mark.parametrize("profile,rss", [("shaped", False), ("shaped", True), ("nopenalty", False), ("nopenalty", True)])
def test_player_equals_the_four_call_loop(pkg, dev, profile, rss, B):
    """Mid-game crowded boards with dead boards planted in front (`midgame` of the row-tuple player's test), then 200
    steps played twice: by play_rollout in launches of 1 + 63 + 136 and by evaluate.play_legal_moves on a second env
    with the same boards, seed and counter, on the same agent.  Boards, aux, every statistic and all 8 MiB of W
    (unchanged) are compared; `status` is never written and the training statistics never see the player.  Random
    weights: the unmasked argmax is an illegal move for some lane of the first step already (asserted)."""
    env, dead = P.midgame(pkg, dev, B, profile, rss)
    agent = random_agent(pkg, dev)
    q = agent.q_values(env.boards).cpu().numpy()
    assert_same_bits(q, model_q(base_weights(), env.boards.cpu().numpy()), "the row's definition")
    legal = env.legal_moves().cpu().numpy()
    assert int(((legal >> q.argmax(1)) & 1 == 0).sum()) > 0
    env_loop = P.twin_of(pkg, env)
    agent.status.fill_(0x777)
    train_stats = agent.stats_i.clone(), agent.stats_f.clone()
    for c in P.CUTS:
        agent.play_rollout(env, c)
    st_loop = P.four_call_loop(agent, env_loop, sum(P.CUTS))
    P.sync(dev)
    st = agent.play_stats()
    assert torch.equal(env.boards, env_loop.boards), "boards differ"
    assert torch.equal(env.aux, env_loop.aux), "aux records differ"
    assert env.ctr == env_loop.ctr == P.WARM + sum(P.CUTS)
    assert st["steps"] == st_loop["steps"] == B * sum(P.CUTS) and st["valid_moves"] == st_loop["valid_moves"]
    assert st["episodes"] == st_loop["episodes"] and st["max_tile_hist"] == st_loop["max_tile_hist"]
    assert st["score_sum"] == round(st_loop["mean_score"] * st_loop["episodes"])
    assert st["explored"] == 0 and st["inserts"] == 0 and st["drops"] == 0
    assert_same_bits(agent.weights, base_weights(), "the player wrote to the weights")
    assert torch.equal(agent.stats_i, train_stats[0]) and torch.equal(agent.stats_f, train_stats[1])
    assert int(agent.status.item()) == 0x777, "status: required, never written"
    assert st["episodes"] >= B and st["episodes"] >= dead, "the span must cover the reset path"


@pytest.mark.parametrize("dev", DEVICES)
def test_player_exploration_against_a_model(pkg, O, dev):
    """epsilon = 0.3 against the numpy model of the player's draw contract (`model_actions` of the row-tuple player's
    test) on this learner's rows, through where the actions lead: boards, aux, explored and valid counts."""
    B, steps, eps = 257, 40, 0.3
    env, _ = P.midgame(pkg, dev, B, dead=3)
    agent = random_agent(pkg, dev)
    model = P.twin_of(pkg, env)
    agent.play_rollout(env, 15, epsilon=eps)
    agent.play_rollout(env, steps - 15, epsilon=eps)
    explored = valid = 0
    for _ in range(steps):
        boards = model.boards.cpu().numpy()
        legal = model.legal_moves().cpu().numpy()
        acts, e = P.model_actions(O, model_q(base_weights(), boards), legal, model.seed, model.env_id0, model.ctr, eps)
        explored += e
        valid += int((legal != 0).sum())
        _, _, done, _ = model.step(torch.from_numpy(acts).to(dev))
        model.reset(done)
    P.sync(dev)
    st = agent.play_stats()
    assert torch.equal(env.boards, model.boards) and torch.equal(env.aux, model.aux)
    assert st["explored"] == explored and st["valid_moves"] == valid and st["steps"] == B * steps
    assert 0.2 * B * steps < explored < 0.4 * B * steps
    assert_same_bits(agent.weights, base_weights(), "the player wrote to the weights")


# ---------------------------------------------------------------------------------------------------------------
# 9. checkpoint and promotion
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_checkpoint_resumes_the_run(pkg, dev):
    """state_dict -> load_state_dict round-trips bit for bit, and 120 steps, a checkpoint, a fresh agent and env, 80
    more == 200 uninterrupted steps at B = 1 (one lane: a learning run is a function of its inputs) in all of W,
    boards, aux, statistics, counters and epsilon."""
    def run(cuts):
        env = P.make_env(pkg, dev, 1)
        agent = make_agent(pkg, dev, eps=0.9, epochs=10)
        for k, steps in enumerate(cuts):
            agent.fused_rollout(env, steps)
            agent.decay_exploration(k)
            yield env, agent

    for env, agent in run([120, 80]):
        pass
    whole = P.learner_state(agent, env)
    (env1, agent1), = run([120])
    sd, esd = agent1.state_dict(), env1.state_dict()
    assert sd["kind"] == "line_tuple" and sd["board_size"] == 4 and sd["weights"].device.type == "cpu"
    assert sd["weights"].dtype == torch.float32 and tuple(sd["weights"].shape) == (8, 65536, 4)
    assert set(sd) >= {"lr", "gamma", "schedule", "seed", "env_id0", "ctr", "stats_i", "stats_f"}
    assert bool(sd["weights"][:4].any()) and bool(sd["weights"][4:].any())
    env2 = P.make_env(pkg, dev, 1, seed=1, id0=2)
    agent2 = make_agent(pkg, dev, eps=0.1, seed=1, id0=2, epochs=10)
    agent2.load_state_dict(sd)
    env2.load_state_dict(esd)
    P.assert_same_state(P.learner_state(agent2, env2), P.learner_state(agent1, env1))      # the round trip
    agent2.fused_rollout(env2, 80)
    agent2.decay_exploration(1)
    P.sync(dev)
    P.assert_same_state(P.learner_state(agent2, env2), whole)


@pytest.mark.parametrize("dev", DEVICES)
def test_a_wrong_checkpoint_writes_nothing(pkg, dev):
    """Every other kind, shape and dtype is refused before anything is written -- by load_state_dict and by
    load_row_tuple -- and BatchedRowTupleAgent and the hash-table agent refuse a line-tuple checkpoint."""
    env, agent = P.make_env(pkg, dev, 64), make_agent(pkg, dev)
    agent.fused_rollout(env, 20)
    good = agent.state_dict()
    before = P.learner_state(agent, env)
    rt = P.make_agent(pkg, dev)
    rt_sd = rt.state_dict()
    ht = pkg.BatchedQLearningAgent(10, capacity_log2=12, device="cpu", placement="plain")
    marked = dict(good, weights=good["weights"] + 1.0, ctr=999, stats_i=good["stats_i"] + 1)
    wrong = [dict(marked, weights=marked["weights"].double()), dict(marked, weights=marked["weights"][:4]),
             dict(marked, weights=marked["weights"][:, :4096]), dict(marked, weights=marked["weights"].numpy()),
             dict(marked, board_size=5), dict(marked, stats_i=marked["stats_i"].int()),
             dict(marked, stats_f=marked["stats_f"][:2]), {k: v for k, v in marked.items() if k != "kind"},
             dict(marked, kind="row_tuple"), dict(rt_sd, ctr=999), ht.state_dict()]
    for bad in wrong:
        with pytest.raises(ValueError):
            agent.load_state_dict(bad)
        P.sync(dev)
        P.assert_same_state(P.learner_state(agent, env), before)
    rt_marked = dict(rt_sd, weights=rt_sd["weights"] + 1.0, ctr=999)
    for bad in (marked, dict(rt_marked, weights=marked["weights"]), dict(rt_marked, weights=rt_marked["weights"].double()),
                dict(rt_marked, kind="line_tuple"), dict(rt_marked, stats_i=rt_sd["stats_i"].int()), ht.state_dict()):
        with pytest.raises(ValueError):
            agent.load_row_tuple(bad)
        P.sync(dev)
        P.assert_same_state(P.learner_state(agent, env), before)
    rt_before = bits(rt.weights).copy()
    with pytest.raises(ValueError):
        rt.load_state_dict(marked)                                       # unchanged: refuses what it refused
    with pytest.raises(ValueError, match="BatchedLineTupleAgent"):
        ht.load_state_dict(good)
    assert np.array_equal(bits(rt.weights), rt_before) and rt.ctr == 0
    agent.load_state_dict(marked)
    assert agent.ctr == 999 and torch.equal(agent.weights.cpu(), marked["weights"])


@pytest.mark.parametrize("dev", DEVICES)
def test_promotion_of_a_row_tuple_checkpoint(pkg, dev):
    """load_row_tuple: the row-tuple weights in features 0..3 bit for bit, features 4..7 zero, schedule, counters and
    statistics taken; q_values equals the row-tuple agent's AS VALUES on 1000 mid-game boards (the column half adds
    +0.0, so only a -0.0 may change its sign bit); and the promoted learner goes on learning, columns included."""
    rt = P.agent_with(pkg, dev, "trained", eps=0.4)
    rt.ctr, rt.lr = 300, 0.05
    rt.decay_exploration(0)
    rt.stats_i += 3
    sd = rt.state_dict()
    agent = make_agent(pkg, dev, seed=1, id0=2)
    agent.weights.fill_(9.0)                                             # stale columns must not survive
    agent.load_row_tuple(sd)
    assert torch.equal(P.bits(agent.weights[:4]), P.bits(rt.weights)) and not bool(agent.weights[4:].any())
    assert (agent.ctr, agent.seed, agent.env_id0, agent.lr, agent.gamma) == (300, rt.seed, rt.env_id0, 0.05, rt.gamma)
    assert vars(agent.schedule) == vars(rt.schedule) and agent.epsilon == rt.epsilon
    assert torch.equal(agent.stats_i, rt.stats_i) and torch.equal(agent.stats_f, rt.stats_f)
    env, _ = P.midgame(pkg, dev, 1000)
    env.ctr = 300
    q, q_rt = agent.q_values(env.boards).cpu().numpy(), rt.q_values(env.boards).cpu().numpy()
    assert np.array_equal(q, q_rt) and np.abs(q_rt).max() > 0
    assert_same_bits(q + F32(0.0), q_rt + F32(0.0), "the rows after promotion")
    assert agent.state_dict()["kind"] == "line_tuple"
    agent.fused_rollout(env, 5)
    assert bool(agent.weights[4:].any())
