"""The afterstate value learner on the line features (V = float32 [8, 65536]): the six entry points q2048_av_value,
q2048_av_lookup, q2048_av_choose, q2048_av_update, q2048_av_fused_rollout and q2048_av_play_rollout against a numpy model,
and BatchedAfterstateAgent's checkpoint.  (The scripts: test_afterstate_scripts.py.)

Which test executes which kernel (device) / function (CPU twin):
  k_av_value          test_value_and_lookup_at_the_edges, test_65536_boards
  k_av_lookup         test_value_and_lookup_at_the_edges, test_lookup_reads_each_feature_at_the_moved_board,
                      test_lookup_on_boards_with_one_move_none_and_merges, test_65536_boards
  k_av_choose         test_choose_greedy_ties_and_illegal_maxima, test_choose_at_the_edges, test_65536_boards
  k_av_update         test_update_where_lanes_cannot_race
  k_av_fused_rollout  test_fused_rollout_with_frozen_weights, test_fused_rollout_one_lane_many_steps (the carried-entry
                      rule), test_fused_rollout_one_learning_step, test_racing_learning_at_65536_boards_properties
  k_eval_play_rollout<AvEvalOf, E>   test_player_equals_the_four_call_loop, test_player_exploration_against_a_model
  the argument checks test_abi, test_argument_errors_need_no_device, test_refused_calls_write_nothing

The model (model_idx of the line-tuple test, model_v, model_eval, model_best, model_update) is plain numpy, takes the move
from the oracle (`oracle.move`: moved board, merge score, "changed") and shares no code with csrc/.  Every comparison is
exact: integers, bytes, and float32 values as bit patterns.  There is no tolerance: v is a fixed chain of float32
additions, q_a one more float32 addition of an integer below 2^24, the TD step one float64 expression rounded once, and a
contraction of (gamma * best) * live - v into an fma cannot change it because live is 0.0 or 1.0.  Every case runs on the
CPU twin ("cpu") and on the GPU."""
import os

import numpy as np
import pytest
import torch

import test_line_tuple as LT
import test_row_tuple_kernels as K
import test_row_tuple_player as P

REPO = P.REPO
DEVICES = LT.DEVICES
EDGES = LT.EDGES
ROOM, Q_CANARY, A_CANARY, BAD_ACTION = K.ROOM, K.Q_CANARY, K.A_CANARY, K.BAD_ACTION
ERR_NULL, ERR_SIZE, ERR_ALIGN, ERR_RANGE, ERR_FLAGS = -1, -2, -3, -6, -7
F32 = np.float32
NAMES = ("q2048_av_value", "q2048_av_lookup", "q2048_av_choose", "q2048_av_update", "q2048_av_fused_rollout",
         "q2048_av_play_rollout")
lib, t8, t32, bits, assert_same_bits, model_idx = K.lib, K.t8, K.t32, K.bits, K.assert_same_bits, LT.model_idx


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def model_v(V, boards):
    """v(x) = ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7)), e_f = V[f, idx_f(x)], in float32 -> float32 [B]"""
    idx = model_idx(boards)
    e = [V[f, idx[:, f]] for f in range(8)]
    assert all(x.dtype == F32 for x in e)
    return ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]))


_MOVES = {}


def model_moves(O, boards):
    """The oracle's move for the four actions -> (moved uint8 [B, 4, 16], score int64 [B, 4], legal bool [B, 4]); one
    oracle call per distinct (board, action), remembered."""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 16)
    B = len(boards)
    moved, score, legal = np.empty((B, 4, 16), np.uint8), np.empty((B, 4), np.int64), np.empty((B, 4), bool)
    for i in range(B):
        key = boards[i].tobytes()
        hit = _MOVES.get(key)
        if hit is None:
            hit = [O.move(boards[i], a) for a in range(4)]
            _MOVES[key] = hit
        for a in range(4):
            moved[i, a], score[i, a], legal[i, a] = hit[a]
    return moved, score, legal


def model_eval(O, V, boards, moves=None):
    """q_a = float32(score_a) + v(c_a) -> (q float32 [B, 4], legal bool [B, 4], moved boards)"""
    moved, score, legal = moves if moves is not None else model_moves(O, boards)
    assert score.max(initial=0) < 1 << 24
    q = np.stack([score[:, a].astype(F32) + model_v(V, moved[:, a]) for a in range(4)], axis=1)
    assert q.dtype == F32
    return q, legal, moved


def model_greedy(q, legal):
    """The first maximum over the legal moves, strict >; action 0 without a legal move -> int [B]"""
    act = np.zeros(len(q), np.int64)
    for i in range(len(q)):
        have = False
        for a in range(4):
            if legal[i, a] and (not have or q[i, a] > q[i, act[i]]):
                act[i], have = a, True
    return act


def model_best(q, legal):
    """best(s) = q at the greedy legal move, 0.0 without one -> float32 [B]"""
    g = model_greedy(q, legal)
    return np.where(legal.any(axis=1), q[np.arange(len(q)), g], F32(0.0)).astype(F32)


def mask_of(legal):
    return (legal * np.array([1, 2, 4, 8])).sum(axis=1).astype(np.uint8)


def model_update(O, V, s, actions, s2, done, lr, gamma, inplace=False):
    """The TD step, lane after lane on one array.  -> (values afterwards, status word, int [B, 8] written indices or -1)"""
    V, status = (V if inplace else V.copy()), 0
    written = np.full((len(s), 8), -1, np.int64)
    for i in range(len(s)):
        a = int(actions[i])
        if a > 3:
            status |= BAD_ACTION
            continue
        x, _, legal = O.move(s[i], a)
        if not legal:
            continue
        q2, legal2, _ = model_eval(O, V, s2[i:i + 1])
        live = 1.0 if (not done[i]) and legal2.any() else 0.0
        target = (gamma * float(model_best(q2, legal2)[0])) * live                    # float64
        d = F32((lr * 0.125) * (target - float(model_v(V, x[None])[0])))             # rounded once
        idx = model_idx(x[None])[0]
        for f in range(8):
            V[f, idx[f]] = F32(V[f, idx[f]] + d)
        written[i] = idx
    return V, status, written


def entry_sets(O, s, a, s2, fused=False):
    """(read set, write set) of one lane of the TD step, as the model's f * 65536 + idx.  `fused`: the step of the fused
    learner, which also evaluates s itself (all four candidates) where the four-call loop has chosen before any update."""
    reads = {int(f * 65536 + i) for c in model_moves(O, s2[None])[0][0] for f, i in enumerate(model_idx(c[None])[0])}
    if fused:
        reads |= {int(f * 65536 + i) for c in model_moves(O, s[None])[0][0] for f, i in enumerate(model_idx(c[None])[0])}
    writes = set()
    if a <= 3:
        x, _, legal = O.move(s, a)
        if legal:
            writes = {int(f * 65536 + i) for f, i in enumerate(model_idx(x[None])[0])}
    return reads | writes, writes


def entry_sets_many(O, s, a, s2, fused=False):
    """`entry_sets` for many lanes at once (the same sets; the indices of all candidates in one numpy pass)."""
    n, off = len(s), np.arange(8) * 65536
    moved_s, _, legal_s = model_moves(O, s)
    at = lambda boards: (model_idx(boards.reshape(-1, 16)) + off).reshape(n, -1)      # noqa: E731
    reads = np.concatenate([at(model_moves(O, s2)[0])] + ([at(moved_s)] if fused else []), axis=1)
    ok = a <= 3
    act = np.where(ok, a, 0)
    wrote = ok & legal_s[np.arange(n), act]
    writes = at(moved_s[np.arange(n), act])
    out = []
    for i in range(n):
        w = set(writes[i].tolist()) if wrote[i] else set()
        out.append((set(reads[i].tolist()) | w, w))
    return out


def conflicts(sets):
    """Lanes whose write set meets an earlier lane's read or write set, or whose read set meets an earlier write set."""
    seen_r, seen_w, bad = set(), set(), []
    for i, (r, w) in enumerate(sets):
        if (w & seen_r) or (r & seen_w):
            bad.append(i)
            continue
        seen_r |= r
        seen_w |= w
    return bad


# ---------------------------------------------------------------------------------------------------------------
# the entry points, through ctypes alone
# ---------------------------------------------------------------------------------------------------------------
def av_value(L, dev, weights, boards):
    B = len(boards)
    out = torch.full((B + ROOM,), Q_CANARY - (1 << 32), dtype=torch.int32, device=dev)
    tb = t8(dev, boards)
    assert L.q2048_av_value(weights.data_ptr(), tb.data_ptr(), B, out.data_ptr(), None) == 0
    out = out.cpu().numpy().view(np.uint32)
    return out[:B], out[B:]


def av_lookup(L, dev, weights, boards):
    B = len(boards)
    out = torch.full((B + ROOM, 4), Q_CANARY - (1 << 32), dtype=torch.int32, device=dev)
    tb = t8(dev, boards)
    assert L.q2048_av_lookup(weights.data_ptr(), tb.data_ptr(), B, out.data_ptr(), None) == 0
    out = out.cpu().numpy().view(np.uint32)
    return out[:B], out[B:]


def av_choose(L, dev, weights, boards, eps, seed=0, env_id0=0, ctr=0):
    B = len(boards)
    out = torch.full((B + ROOM,), A_CANARY, dtype=torch.uint8, device=dev)
    tb = t8(dev, boards)
    assert L.q2048_av_choose(weights.data_ptr(), tb.data_ptr(), B, float(eps), seed, env_id0, ctr, out.data_ptr(),
                             None) == 0
    out = out.cpu().numpy()
    return out[:B], out[B:]


_SHARED = {}


def base_values():
    """Random normal float32 [8, 65536] (scale 4: it outweighs most merge scores), built once; nobody writes it."""
    if "v" not in _SHARED:
        v = (4.0 * np.random.default_rng(22).standard_normal((8, 65536))).astype(F32)
        v.setflags(write=False)
        _SHARED["v"] = v
    return _SHARED["v"]


def midgame(O):
    """The 65,536 mid-game boards of the row-tuple test with the oracle's four moves of each, computed once."""
    if "mid" not in _SHARED:
        boards, _ = K.midgame_boards(O)
        moves = model_moves(O, boards)
        for a in moves:
            a.setflags(write=False)
        _SHARED["mid"] = (boards, moves)
    return _SHARED["mid"]


def crowded():
    """20,000 late mid-game boards: tiles 2..32768 uniformly, two empty cells.  The pool for the tests whose lanes must
    not race: the oracle's mid-game boards above share their hot entries (an empty line, a line with one tile) among
    most of the batch, and the acceptance rule finds about twenty lanes that write among 20,000 of them; here a line is
    one of 15^4, and a thousand lanes are found among a few thousand candidates."""
    if "crowded" not in _SHARED:
        rng = np.random.default_rng(23)
        b = rng.integers(1, 16, size=(20000, 16), dtype=np.uint8)
        for i in range(len(b)):
            b[i, rng.choice(16, 2, replace=False)] = 0
        b.setflags(write=False)
        _SHARED["crowded"] = b
    return _SHARED["crowded"]


def make_agent(pkg, dev, eps=0.3, lr=0.1, gamma=0.95, seed=P.SEED, id0=P.ID0, epochs=100):
    return pkg.BatchedAfterstateAgent(epochs, learning_rate=lr, discount_factor=gamma, exploration_rate=eps, seed=seed,
                                      env_id0=id0, device=dev)


# ---------------------------------------------------------------------------------------------------------------
# 1. ABI and argument errors
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
    assert pkg.BatchedAfterstateAgent is __import__("q2048_amd").BatchedAfterstateAgent
    assert issubclass(pkg.BatchedAfterstateAgent, pkg.BatchedLineTupleAgent)


def entry_points(L):
    a = [0x1000 * (k + 1) for k in range(8)]
    nan = float("nan")
    # name: (function, good arguments, required pointers, 16-byte aligned pointers, position of B, {scalar position: refused})
    return {
        "av_value": (L.q2048_av_value, [a[0], a[1], 64, a[2], None], (0, 1, 3), (0, 1, 3), 2, {}),
        "av_lookup": (L.q2048_av_lookup, [a[0], a[1], 64, a[2], None], (0, 1, 3), (0, 1, 3), 2, {}),
        "av_choose": (L.q2048_av_choose, [a[0], a[1], 64, 0.3, 7, 50, 3, a[2], None], (0, 1, 7), (0, 1), 2,
                      {3: (-0.1, 1.5, nan)}),
        "av_update": (L.q2048_av_update, [a[0], a[1], a[2], a[3], a[4], 64, 0.1, 0.97, a[5], None],
                      (0, 1, 2, 3, 4, 8), (0, 1, 3), 5, {6: (nan,), 7: (nan,)}),
        "av_fused_rollout": (L.q2048_av_fused_rollout, [a[0], a[1], a[2], 64, 2, 0.3, 0.1, 0.97, 3, 50, 0, None, None,
                                                        a[3], None],
                             (0, 1, 2, 13), (0, 1, 2), 3, {5: (-0.1, 1.5, nan), 6: (nan,), 7: (nan,)}),
    }


@pytest.mark.parametrize("which", ["hip", "host"])
def test_argument_errors_need_no_device(pkg, which):
    """The documented order -- B, (flags,) NULL, alignment, (steps,) the scalars -- on both libraries, with made-up
    aligned addresses: every refused call also carries the errors that come later in the order, and nothing behind
    the addresses is touched (B == 0 and steps == 0 are no-ops)."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    nan, big = float("nan"), (2 ** 31 - 1) * 256 + 1
    table = entry_points(L)
    for name, (fn, good, pointers, aligned, b_pos, scalars) in table.items():
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
    fn, good = table["av_fused_rollout"][:2]
    for steps, eps, code in ((-1, nan, ERR_SIZE), ((1 << 30) + 1, nan, ERR_SIZE), (0, 0.3, 0), (0, nan, ERR_RANGE)):
        args = list(good)
        args[4], args[5] = steps, eps                                   # steps before epsilon
        assert fn(*args) == code, f"av_fused_rollout: steps = {steps}"
    ok = P.argument_errors(L.q2048_av_play_rollout, 0x1000, 0x2000, 0x3000, 0x4000)
    for bit in (N.FLAG_INDEPENDENT, N.FLAG_SYMMETRIC, N.FLAG_SINGLE_ENV, N.FLAG_TD_CAS, N.FLAG_PLAY_ONLY, N.FLAG_NO_LEARN,
                N.FLAG_NO_NEW_ROWS, N.FLAG_LINE_SUMMARY, 1 << 8, 1 << 23, 1 << 30, 1 << 31):
        assert ok(flags=bit) == ERR_FLAGS and ok(flags=bit | N.FLAG_ENV_DQN | N.FLAG_RESET_SHAPING) == ERR_FLAGS, bit
    assert ok(B=0) == 0 and ok(steps=0) == 0
    assert ok(B=0, boards=None) == ERR_NULL and ok(steps=0, weights=0x3008) == ERR_ALIGN
    assert ok(B=0, flags=N.FLAG_INDEPENDENT) == ERR_FLAGS


@pytest.mark.parametrize("dev", DEVICES)
def test_refused_calls_write_nothing(pkg, dev):
    """Each entry point refused for its LAST check (a scalar out of range; a misaligned output where it has no scalar)
    on real buffers: weights, boards, aux, outputs, statistics and status keep every byte."""
    L, B = lib(pkg, dev), 64
    nan = float("nan")
    V = t32(dev, base_values())
    boards = t8(dev, K.random_boards(np.random.default_rng(1), B))
    aux = torch.full((B, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    out = torch.full((B * 4 + 8,), 0x6B6B6B6B, dtype=torch.int32, device=dev)
    acts = torch.full((B,), 2, dtype=torch.uint8, device=dev)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    si, sf = torch.full((64,), 7, dtype=torch.int64, device=dev), torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((1,), 0x777, dtype=torch.int32, device=dev)
    everything = (V, boards, aux, out, acts, done, si, sf, status)
    before = [t.clone() for t in everything]
    p = lambda t: t.data_ptr()      # noqa: E731
    calls = [
        L.q2048_av_value(p(V), p(boards), B, p(out) + 8, None),
        L.q2048_av_lookup(p(V), p(boards), B, p(out) + 8, None),
        L.q2048_av_choose(p(V), p(boards), B, 1.5, 1, 0, 0, p(acts), None),
        L.q2048_av_update(p(V), p(boards), p(acts), p(boards), p(done), B, 0.1, nan, p(status), None),
        L.q2048_av_fused_rollout(p(boards), p(aux), p(V), B, 3, 0.3, nan, 0.9, 1, 0, 0, p(si), p(sf), p(status), None),
        L.q2048_av_play_rollout(p(boards), p(aux), p(V), B, 3, nan, 1, 0, 0, 0, p(si), p(sf), p(status), None),
        L.q2048_av_play_rollout(p(boards), p(aux), p(V), B, 3, 0.0, 1, 0, 0, 1 << 8, p(si), p(sf), p(status), None),
    ]
    P.sync(dev)
    assert calls == [ERR_ALIGN, ERR_ALIGN, ERR_RANGE, ERR_RANGE, ERR_RANGE, ERR_RANGE, ERR_FLAGS]
    for t, b in zip(everything, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "a refused call wrote"


# ---------------------------------------------------------------------------------------------------------------
# 2. av_value and av_lookup
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
def test_value_and_lookup_at_the_edges(pkg, O, dev, B):
    """Random values over all 2 MiB.  av_value on random cells 0..31: a cell of 16..31 reads the entry of its low nibble.
    av_lookup on random cells 0..15 (two 15s merge into a 16, which aliases to 0 -- the model masks too).  The records
    beyond B keep their canary; the weights are not written."""
    L, V = lib(pkg, dev), base_values()
    rng = np.random.default_rng(100 + B)
    wide = rng.integers(0, 32, size=(B, 16), dtype=np.uint8)
    wide[0, 6] = 16 + 5
    want_v = model_v(V, wide)
    assert_same_bits(want_v, model_v(V, wide & 15), "the model's own mask")
    weights = t32(dev, V)
    got, tail = av_value(L, dev, weights, wide)
    assert_same_bits(got.view(F32), want_v, f"values, B = {B}")
    assert (tail == np.uint32(Q_CANARY)).all(), "values written beyond B"

    boards = K.random_boards(rng, B)
    q, legal, moved = model_eval(O, V, boards)
    got, tail = av_lookup(L, dev, weights, boards)
    assert_same_bits(got.view(F32), q, f"rows, B = {B}")
    assert (tail == np.uint32(Q_CANARY)).all(), "rows written beyond B"
    assert_same_bits(weights, V, "a lookup wrote the weights")
    if B >= 63:      # teeth: the row is neither v(s) four times nor v(c_a) without the score
        v_s = model_v(V, boards)
        assert (bits(q) != bits(v_s)[:, None]).all(axis=1).any() and model_moves(O, boards)[1].max() > 0


@pytest.mark.parametrize("dev", DEVICES)
def test_lookup_reads_each_feature_at_the_moved_board(pkg, O, dev):
    """For each f the values are non-zero in table f only, and no board equals its transpose or a mirror image: a kernel
    that reads a column index from a row table, a column from the bottom, or the indices of s instead of c_a, returns
    another row."""
    L, B = lib(pkg, dev), 257
    boards = np.random.default_rng(150).integers(0, 12, size=(B, 16), dtype=np.uint8)
    g = boards.reshape(B, 4, 4)
    assert (g != g.transpose(0, 2, 1)).any(axis=(1, 2)).all() and (g != g[:, :, ::-1]).any(axis=(1, 2)).all()
    moves = model_moves(O, boards)
    moved, score, legal = moves
    for f in range(8):
        V = np.zeros((8, 65536), dtype=F32)
        V[f] = base_values()[f]
        q, _, _ = model_eval(O, V, boards, moves)
        at_s = score.astype(F32) + model_v(V, boards)[:, None]                       # v read at s, not at c_a
        mt = moved.reshape(B, 4, 4, 4).transpose(0, 1, 3, 2).reshape(B, 4, 16)       # c_a transposed
        at_t = np.stack([score[:, a].astype(F32) + model_v(V, mt[:, a]) for a in range(4)], axis=1)
        assert (bits(at_s) != bits(q)).any(axis=1).mean() > 0.9 and (bits(at_t) != bits(q)).any(axis=1).mean() > 0.9
        got, _ = av_lookup(L, dev, t32(dev, V), boards)
        assert_same_bits(got.view(F32), q, f"feature {f}")


def special_boards():
    """Boards with exactly one legal move (each of the four), with none, and with merges of known score."""
    out = [P.one_move_board(a) for a in range(4)]
    out.append(P.DEAD.numpy().copy())
    merge = np.zeros(16, np.uint8)
    merge[[0, 1, 4, 5]] = [3, 3, 3, 2]                 # left / right merge 8 + 8 in row 0; up / down merge 8 + 8 in column 0
    out.append(merge)
    big = np.array([5, 5, 6, 6, 1, 2, 1, 2, 7, 0, 0, 7, 0, 0, 0, 0], np.uint8)      # left: 64 + 128 + 256
    out.append(big)
    return np.stack(out).astype(np.uint8)


@pytest.mark.parametrize("dev", DEVICES)
def test_lookup_on_boards_with_one_move_none_and_merges(pkg, O, dev):
    """Exactly one legal move (the three others give 0 + v(s) bit for bit), no legal move (four times v(s)), and moves
    that merge: score_a is added and v is read at the moved board, not at s.  The same boards through av_choose at
    epsilon 0 and 1: the one legal move, or action 0 where there is none."""
    L, V = lib(pkg, dev), base_values()
    boards = special_boards()
    moved, score, legal = model_moves(O, boards)
    assert [int(x.sum()) for x in legal[:5]] == [1, 1, 1, 1, 0] and [int(np.argmax(x)) for x in legal[:4]] == [0, 1, 2, 3]
    assert score[5].tolist() == [16, 16, 16, 16] and score[6, 0] == 64 + 128 + 256
    q, _, _ = model_eval(O, V, boards)
    v_s = model_v(V, boards)
    assert (bits(q)[~legal] == np.broadcast_to(bits(v_s)[:, None], q.shape)[~legal]).all()
    assert (bits(q[5]) != bits(F32(16.0) + v_s[5])).all(), "the merging moves do not tell c_a from s"
    weights = t32(dev, V)
    got, _ = av_lookup(L, dev, weights, boards)
    assert_same_bits(got.view(F32), q, "special boards")
    want = model_greedy(q, legal)
    for eps in (0.0, 1.0):
        got, tail = av_choose(L, dev, weights, boards[:5], eps, 3, 9, 1)
        assert got.tolist() == want[:5].tolist() == [0, 1, 2, 3, 0], f"epsilon = {eps}"
        assert (tail == A_CANARY).all()


@pytest.mark.parametrize("dev", DEVICES)
def test_65536_boards(pkg, O, dev):
    """256 full blocks of mid-game boards (hot entries shared by most of the batch, as in a rollout): values and rows bit
    for bit, greedy actions equal, and the read-only pass leaves V bit-identical."""
    L, V = lib(pkg, dev), base_values()
    boards, moves = midgame(O)
    q, legal, _ = model_eval(O, V, boards, moves)
    weights = t32(dev, V)
    got, tail = av_value(L, dev, weights, boards)
    assert_same_bits(got.view(F32), model_v(V, boards), "65,536 values")
    assert (tail == np.uint32(Q_CANARY)).all()
    got, tail = av_lookup(L, dev, weights, boards)
    assert_same_bits(got.view(F32), q, "65,536 rows")
    assert (tail == np.uint32(Q_CANARY)).all(), "rows written beyond B"
    greedy = model_greedy(q, legal).astype(np.uint8)
    assert np.bincount(greedy, minlength=4).min() > 0 and (~legal).any()
    got, tail = av_choose(L, dev, weights, boards, 0.0, 41, 0, 40)
    assert np.array_equal(got, greedy), f"{int((got != greedy).sum())} greedy actions differ"
    assert (tail == A_CANARY).all(), "actions written beyond B"
    assert_same_bits(weights, V, "a read-only pass wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 3. av_choose
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_choose_greedy_ties_and_illegal_maxima(pkg, O, dev):
    """(a) Zero values: q_a = score_a exactly, so legal moves tie two ways and four ways at the maximum (counted from
    the model); the first legal maximum wins.  (b) Random values with +50 planted on the eight entries of s on lanes
    that have an illegal move: the illegal moves read 0 + v(s) = the largest q of the row, and must not be played."""
    L, B = lib(pkg, dev), 1000
    boards = midgame(O)[0][:B]
    moves = tuple(m[:B] for m in midgame(O)[1])
    q, legal, _ = model_eval(O, np.zeros((8, 65536), F32), boards, moves)
    top = np.where(legal, q, -np.inf)
    ties = ((top == top.max(axis=1, keepdims=True)) & legal).sum(axis=1)
    assert (ties == 2).sum() > 10 and (ties == 3).sum() > 10 and (ties == 4).sum() > 10     # (a unique maximum: part (b))
    want = model_greedy(q, legal)
    assert (want[ties == 2] > 0).any(), "every two-way tie is won by action 0"
    got, tail = av_choose(L, dev, torch.zeros((8, 65536), dtype=torch.float32, device=dev), boards, 0.0)
    assert np.array_equal(got, want) and (tail == A_CANARY).all()

    V = base_values().copy()
    lanes = np.flatnonzero(~legal.all(axis=1) & legal.any(axis=1))[:40]
    idx = model_idx(boards)
    for i in lanes:
        V[np.arange(8), idx[i]] = 50.0
    q, legal, _ = model_eval(O, V, boards, moves)
    want = model_greedy(q, legal)
    held = [i for i in lanes if not legal[i, int(np.argmax(q[i]))]]
    assert len(held) > 10, "too few lanes whose largest q belongs to an illegal move"
    got, _ = av_choose(L, dev, t32(dev, V), boards, 0.0)
    assert np.array_equal(got, want)
    assert all(legal[i, got[i]] for i in held)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
def test_choose_at_the_edges(pkg, O, dev, B):
    """epsilon = 0: the model's first legal maximum.  epsilon = 0.3 with (seed, env_id0, ctr) = (7, 2^33 + 5, 3): the
    player's draw contract (`model_actions` of the row-tuple player's test) on this learner's rows."""
    L, V = lib(pkg, dev), base_values()
    boards = midgame(O)[0][1000:1000 + B]
    moves = tuple(m[1000:1000 + B] for m in midgame(O)[1])
    q, legal, _ = model_eval(O, V, boards, moves)
    weights = t32(dev, V)
    greedy = model_greedy(q, legal).astype(np.uint8)
    got, tail = av_choose(L, dev, weights, boards, 0.0)
    assert np.array_equal(got, greedy), f"greedy actions differ on lanes {np.flatnonzero(got != greedy)[:8].tolist()}"
    assert (tail == A_CANARY).all(), "actions written beyond B"
    eps, seed, id0, ctr = 0.3, 7, (1 << 33) + 5, 3
    want, explored = P.model_actions(O, q, mask_of(legal), seed, id0, ctr, eps)
    if B >= 63:
        assert 0 < explored < B and (want != greedy).any()
    got, tail = av_choose(L, dev, weights, boards, eps, seed, id0, ctr)
    assert np.array_equal(got, want), f"actions differ on lanes {np.flatnonzero(got != want)[:8].tolist()}"
    assert (tail == A_CANARY).all(), "actions written beyond B"
    assert_same_bits(weights, V, "choosing wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 4. av_update where lanes cannot race
# ---------------------------------------------------------------------------------------------------------------
def spawned(rng, board):
    """The board with a 2 or a 4 in one of its empty cells (any: the test needs a plausible s', not the env's)."""
    b = board.copy()
    empty = np.flatnonzero(b == 0)
    if len(empty):
        b[rng.choice(empty)] = 1 if rng.random() < 0.9 else 2
    return b


def nonracing_transitions(O, rng, B):
    """Candidate transitions from the `crowded` mid-game boards -- s a board, a uniform (every 7th candidate 7, a bad
    action; every 11th a board with one legal move and another action), s' = the moved board with a spawn (s itself for
    an illegal move; every 5th candidate the dead board) -- accepted lane by lane if the write set is disjoint from
    every earlier read and write set and the read set from every earlier write set."""
    boards = crowded()
    order = rng.permutation(len(boards))
    s, a, s2, seen_r, seen_w = [], [], [], set(), set()
    for n, c in enumerate(order):
        board = boards[c]
        act = 7 if n % 7 == 3 else int(rng.integers(0, 4))
        if n % 11 == 5:
            board, act = P.one_move_board(n % 4), (n + 1) % 4
        x = O.move(board, act)[0] if act <= 3 else board
        nxt = P.DEAD.numpy().copy() if n % 5 == 2 else spawned(rng, x)
        r, w = entry_sets(O, board, act, nxt)
        if (w & seen_r) or (r & seen_w):
            continue
        seen_r |= r
        seen_w |= w
        s.append(board); a.append(act); s2.append(nxt)      # noqa: E702
        if len(s) == B:
            break
    return np.stack(s), np.array(a, np.uint8), np.stack(s2)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [65, 257, 1000])
def test_update_where_lanes_cannot_race(pkg, O, dev, B):
    """No lane reads or writes an entry another lane writes (by construction, asserted), so the result does not depend
    on the order of the lanes and the sequential model is the specification.  All 2 MiB are compared: exactly 8 values
    per lane with a legal action moved, none for an illegal or a bad action (both present); done = 1 and a dead s'
    both give target 0 (both present, and both told from the live target by the model)."""
    L, V = lib(pkg, dev), base_values()
    rng = np.random.default_rng(300 + B)
    s, actions, s2 = nonracing_transitions(O, rng, B)
    assert len(s) == B, f"only {len(s)} lanes that cannot race"
    assert not conflicts(entry_sets_many(O, s, actions.astype(np.int64), s2))
    done = (rng.random(B) < 0.3).astype(np.uint8)
    lr, gamma = 0.1, 0.97
    want, want_status, written = model_update(O, V, s, actions, s2, done, lr, gamma)
    wrote = written[:, 0] >= 0
    bad = actions > 3
    illegal = ~wrote & ~bad
    dead = (s2 == P.DEAD.numpy()).all(axis=1)
    assert bad.any() and illegal.any() and want_status == BAD_ACTION
    assert (wrote & (done == 1)).any() and (wrote & dead & (done == 0)).any() and (wrote & ~dead & (done == 0)).any()
    assert int((bits(want) != bits(V)).sum()) == 8 * int(wrote.sum())
    alive, _, _ = model_update(O, V, s, actions, s2, np.zeros(B, np.uint8), lr, gamma)
    assert (bits(alive) != bits(want)).sum() >= 8 * int((wrote & (done == 1) & ~dead).sum()) > 0, "done does not show"

    weights, status = t32(dev, V), torch.zeros(1, dtype=torch.int32, device=dev)
    ts, ts2, ta, td = t8(dev, s), t8(dev, s2), t8(dev, actions), t8(dev, done)
    assert L.q2048_av_update(weights.data_ptr(), ts.data_ptr(), ta.data_ptr(), ts2.data_ptr(), td.data_ptr(), B, lr, gamma,
                             status.data_ptr(), None) == 0
    got = weights.cpu().numpy()
    assert int(status.item()) == want_status
    assert_same_bits(got, want, f"B = {B}")
    assert int((bits(got) != bits(V)).sum()) == 8 * int(wrote.sum())
    for t, a in ((ts, s), (ts2, s2), (ta, actions), (td, done)):
        assert np.array_equal(t.cpu().numpy(), a), "an input was written"


# ---------------------------------------------------------------------------------------------------------------
# 5.-7. the fused learner against the four-call loop of the same agent class
# ---------------------------------------------------------------------------------------------------------------
def fused_run(pkg, dev, V, B, launches, seed, id0, eps, lr, gamma, boards=None):
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    agent = make_agent(pkg, dev, eps, lr, gamma, seed, id0)
    agent.weights.copy_(torch.from_numpy(V))
    if boards is not None:
        env.boards.copy_(torch.from_numpy(boards))
    for k in launches:
        agent.fused_rollout(env, k)
    assert agent.check_status() == 0
    return env, agent


def four_call_run(pkg, O, dev, V, B, steps, seed, id0, eps, lr, gamma, boards=None, learn=False, keep=False):
    """choose_action -> env.step -> (model_update on V, mirrored into the agent) -> env.reset(done), `steps` times: the
    loop the fused learner replaces, on entry points the tests above have pinned to the model.  -> (env, V afterwards,
    the statistics the fused learner counts, the transitions)"""
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    agent = make_agent(pkg, dev, eps, lr, gamma, seed, id0)
    V = V.copy()
    agent.weights.copy_(torch.from_numpy(V))
    if boards is not None:
        env.boards.copy_(torch.from_numpy(boards))
    thr = 0 if eps <= 0.0 else int(np.ceil(eps * 4294967296.0))
    st = {"steps": 0, "episodes": 0, "valid_moves": 0, "explored": 0, "score_sum": 0}
    trans = []
    for t in range(steps):
        s = env.boards.cpu().numpy().copy()
        has_move = env.legal_moves().cpu().numpy() != 0
        actions = agent.choose_action(env.boards)
        s2, _, done, _ = env.step(actions)
        s2, a, d = s2.cpu().numpy().copy(), actions.cpu().numpy(), done.cpu().numpy().copy()
        st["steps"] += B
        st["episodes"] += int(d.sum())
        st["valid_moves"] += int((s != s2).any(axis=1).sum())            # a move that changes the board, spawn included
        st["score_sum"] += int(env.score.cpu().numpy()[d].sum())
        if eps > 0.0 and not keep:                                       # explored: the draw is below, and a move exists
            st["explored"] += sum(int(O.draws(seed, id0 + i, t)[0]) < thr and bool(has_move[i]) for i in range(B))
        if learn:
            _, _, written = model_update(O, V, s, a, s2, d, lr, gamma, inplace=True)
            if B > 1:
                agent.weights.copy_(torch.from_numpy(V))
            elif written[0, 0] >= 0:
                f = torch.arange(8)
                agent.weights[f, torch.from_numpy(written[0])] = torch.from_numpy(V[np.arange(8), written[0]]).to(dev)
            trans.append((s, a, s2, d, written))
        elif keep:
            trans.append((s, a, s2, d, None))
        env.reset(done)
    return env, V, st, trans


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B,steps,eps", [(257, 100, 0.3), (1000, 120, 0.0)])
def test_fused_rollout_with_frozen_weights(pkg, O, dev, B, steps, eps):
    """learning_rate = 0: every lane is a function of V alone, so the four-call loop is the specification at any batch
    size.  Launches of 1 and steps - 1 steps: the evaluation carried from step to step, the one gathered again after a
    reset and the first one of a launch all decide actions here.  Boards, aux records and statistics equal the loop's;
    the values are bit for bit what was loaded.  Teeth: on zero values the same run ends on other boards in more than
    half of the lanes."""
    seed, id0, gamma = 17, 1000, 0.97
    V = (4.0 * np.random.default_rng(500 + B).standard_normal((8, 65536))).astype(F32)
    env_loop, _, st_loop, _ = four_call_run(pkg, O, dev, V, B, steps, seed, id0, eps, 0.0, gamma)
    env, agent = fused_run(pkg, dev, V, B, (1, steps - 1), seed, id0, eps, 0.0, gamma)
    st = LT.assert_same_run(env, agent, env_loop, st_loop, f"B = {B}")
    assert st["episodes"] > 0 and (st["explored"] == 0) == (eps == 0.0)
    assert_same_bits(agent.weights, V, "frozen values were written")
    env0, _ = fused_run(pkg, dev, np.zeros_like(V), B, (1, steps - 1), seed, id0, eps, 0.0, gamma)
    differ = int((env0.boards.cpu() != env.boards.cpu()).any(dim=1).sum())
    print(f"zero values end on other boards in {differ} of {B} lanes")
    assert differ > B // 2, f"the values decide the boards of only {differ} of {B} lanes"


@pytest.mark.parametrize("dev", DEVICES)
def test_fused_rollout_one_lane_many_steps(pkg, O, dev):
    """THE CARRIED-ENTRY RULE.  B = 1, lr 0.1, gamma 0.97, epsilon 0.3, 300 steps in launches of 1, 63 and 236: one lane
    is the sequential learner, so the expected values are model_update applied step by step to the transitions of the
    four-call loop (the draws make them the same transitions).  All 2 MiB bit for bit, boards and aux equal.  The fused
    kernel gathers the 32 entries of s' BEFORE it writes c_act and carries them into the next step: an entry at a
    written (feature, index) must take the written value.  The test counts, from the model, the steps (not done) in
    which a candidate of s' shares an index with the written afterstate at a row feature and at a column feature, and
    needs both."""
    seed, id0, eps, lr, gamma, cuts = 5, 77, 0.3, 0.1, 0.97, (1, 63, 236)
    V = (4.0 * np.random.default_rng(700).standard_normal((8, 65536))).astype(F32)
    env_loop, want, st_loop, trans = four_call_run(pkg, O, dev, V, 1, sum(cuts), seed, id0, eps, lr, gamma, learn=True)
    rows = cols = 0
    for s, a, s2, d, written in trans:
        if d[0] or written[0, 0] < 0:
            continue
        cand = model_idx(model_moves(O, s2)[0][0])                                   # [4 candidates, 8]
        shared = (cand == written[0][None, :]).any(axis=0)
        rows += bool(shared[:4].any())
        cols += bool(shared[4:].any())
    print(f"steps on which a carried entry was corrected: {rows} at a row feature, {cols} at a column feature; "
          f"episodes {st_loop['episodes']}")
    assert rows > 0 and cols > 0 and st_loop["episodes"] > 0
    env, agent = fused_run(pkg, dev, V, 1, cuts, seed, id0, eps, lr, gamma)
    LT.assert_same_run(env, agent, env_loop, st_loop, "B = 1")
    assert_same_bits(agent.weights, want, "300 sequential steps")
    assert (bits(want) != bits(V)).sum() > 300


def nonracing_boards(pkg, O, dev, V, B, seed, id0, eps):
    """Boards for one fused learning step whose lanes cannot race.  A lane's transition is a function of its board, its
    position (the draws) and V, so: take B `crowded` boards, run one step of the four-call loop with lr = 0, find the
    lanes that conflict with an earlier lane (the rule of `nonracing_transitions`, on the model's indices; the read set
    of a fused step includes the four candidates of s, which the kernel gathers while other lanes already write), give
    them fresh boards, and repeat until no lane conflicts."""
    if ("nonracing", B) in _SHARED:                  # (found once, on the CPU twin: both devices get the same boards)
        return _SHARED[("nonracing", B)]
    pool, dev = crowded(), "cpu"
    nxt = B
    boards = pool[:B].copy()
    sets, fresh = [None] * B, range(B)
    for _ in range(400):
        _, _, _, trans = four_call_run(pkg, O, dev, V, B, 1, seed, id0, eps, 0.0, 0.0, boards=boards, keep=True)
        s, a, s2, _, _ = trans[0]
        fresh = list(fresh)
        for i, rw in zip(fresh, entry_sets_many(O, s[fresh], a[fresh].astype(np.int64), s2[fresh], fused=True)):
            sets[i] = rw
        fresh = conflicts(sets)
        if not fresh:
            _SHARED[("nonracing", B)] = boards
            return boards
        assert nxt + len(fresh) <= len(pool), "the pool is used up"
        boards[fresh] = pool[nxt:nxt + len(fresh)]
        nxt += len(fresh)
    raise AssertionError("no set of lanes that cannot race was found")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [65, 257, 1000])
def test_fused_rollout_one_learning_step(pkg, O, dev, B):
    """One learning step (lr 0.1, gamma 0.97, epsilon 0.3) on lanes that cannot race: model_update on the transitions of
    the four-call loop is the specification.  All values bit for bit, exactly 8 changed per lane whose move was legal;
    boards, aux and statistics equal."""
    seed, id0, eps, lr, gamma = 23, 4000, 0.3, 0.1, 0.97
    V = (4.0 * np.random.default_rng(600 + B).standard_normal((8, 65536))).astype(F32)
    boards = nonracing_boards(pkg, O, dev, V, B, seed, id0, eps)
    env_loop, want, st_loop, trans = four_call_run(pkg, O, dev, V, B, 1, seed, id0, eps, lr, gamma, boards=boards, learn=True)
    wrote = int((trans[0][4][:, 0] >= 0).sum())
    assert wrote > B // 2 and int((bits(want) != bits(V)).sum()) == 8 * wrote and 0 < st_loop["explored"] < B
    env, agent = fused_run(pkg, dev, V, B, (1,), seed, id0, eps, lr, gamma, boards=boards)
    LT.assert_same_run(env, agent, env_loop, st_loop, f"B = {B}")
    got = agent.weights.cpu().numpy()
    assert_same_bits(got, want, f"B = {B}")


# ---------------------------------------------------------------------------------------------------------------
# 8. the player
# ---------------------------------------------------------------------------------------------------------------
def random_agent(pkg, dev, **kw):
    agent = make_agent(pkg, dev, **kw)
    agent.weights.copy_(torch.from_numpy(base_values().copy()))
    return agent


def midgame_env(pkg, dev, B, profile="shaped", rss=False, dead=5):
    """`midgame` of the row-tuple player's test (its scratch learner warms the aux records up)."""
    return P.midgame(pkg, dev, B, profile, rss, dead)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [65, 1000])
@pytest.mark.parametrize("profile,rss", [("shaped", False), ("shaped", True), ("nopenalty", False), ("nopenalty", True)])
def test_player_equals_the_four_call_loop(pkg, O, dev, profile, rss, B):
    """Mid-game crowded boards with dead boards planted in front, then 200 steps played twice: by play_rollout in
    launches of 1 + 63 + 136 and by evaluate.play_legal_moves (av_lookup, legal_moves, env step, env reset) on a second
    env with the same boards, seed and counter, on the same agent.  Boards, aux, every statistic and all 2 MiB of V
    (unchanged) are compared; `status` is never written and the training statistics never see the player."""
    env, dead = midgame_env(pkg, dev, B, profile, rss)
    agent = random_agent(pkg, dev)
    q = agent.q_values(env.boards).cpu().numpy()
    mq, mlegal, _ = model_eval(O, base_values(), env.boards.cpu().numpy())
    assert_same_bits(q, mq, "the row's definition")
    legal = env.legal_moves().cpu().numpy()
    assert np.array_equal(legal, mask_of(mlegal)) and int(((legal >> q.argmax(1)) & 1 == 0).sum()) > 0
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
    assert_same_bits(agent.weights, base_values(), "the player wrote to the weights")
    assert torch.equal(agent.stats_i, train_stats[0]) and torch.equal(agent.stats_f, train_stats[1])
    assert int(agent.status.item()) == 0x777, "status: required, never written"
    assert st["episodes"] >= B and st["episodes"] >= dead, "the span must cover the reset path"


@pytest.mark.parametrize("dev", DEVICES)
def test_player_exploration_against_a_model(pkg, O, dev):
    """epsilon = 0.3 against the numpy model of the player's draw contract on the model's rows, through where the actions
    lead: boards, aux, explored and valid counts."""
    B, steps, eps = 257, 40, 0.3
    env, _ = midgame_env(pkg, dev, B, dead=3)
    agent = random_agent(pkg, dev)
    model = P.twin_of(pkg, env)
    agent.play_rollout(env, 15, epsilon=eps)
    agent.play_rollout(env, steps - 15, epsilon=eps)
    explored = valid = 0
    for _ in range(steps):
        q, legal, _ = model_eval(O, base_values(), model.boards.cpu().numpy())
        acts, e = P.model_actions(O, q, mask_of(legal), model.seed, model.env_id0, model.ctr, eps)
        explored += e
        valid += int(legal.any(axis=1).sum())
        _, _, done, _ = model.step(torch.from_numpy(acts).to(dev))
        model.reset(done)
    P.sync(dev)
    st = agent.play_stats()
    assert torch.equal(env.boards, model.boards) and torch.equal(env.aux, model.aux)
    assert st["explored"] == explored and st["valid_moves"] == valid and st["steps"] == B * steps
    assert 0.2 * B * steps < explored < 0.4 * B * steps
    assert_same_bits(agent.weights, base_values(), "the player wrote to the weights")


# ---------------------------------------------------------------------------------------------------------------
# 9. racing multi-step learning at the quoted batch size: properties only
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_racing_learning_at_65536_boards_properties(pkg, O, dev):
    """65,536 lanes, epsilon = 1, 4 steps in launches of 1 + 3: an exploring choice does not read the values, so the
    trajectories are exact whatever the racing writes do and equal those of the four-call loop (lr = 0).  From its
    transitions and the oracle's move: the entries some lane's afterstate visited.  The values stay finite, ONLY
    visited entries change, and every step, valid move and exploration is counted."""
    B, steps, seed = 65536, 4, 31
    env = pkg.BatchedGame2048Env(B, seed=seed, device=dev)
    agent = make_agent(pkg, dev, eps=1.0, lr=0.05, gamma=0.9, seed=seed, id0=0)
    agent.fused_rollout(env, 1)
    agent.fused_rollout(env, steps - 1)
    loop_env = pkg.BatchedGame2048Env(B, seed=seed, device=dev)
    loop = make_agent(pkg, dev, eps=1.0, lr=0.0, gamma=0.9, seed=seed, id0=0)
    visited = np.zeros((8, 65536), bool)
    valid = explored = 0
    for _ in range(steps):
        s = loop_env.boards.cpu().numpy().copy()
        explored += int((loop_env.legal_moves() != 0).sum())
        a = loop.choose_action(loop_env.boards)
        _, _, done, _ = loop_env.step(a)
        a = a.cpu().numpy()
        moved, _, legal = model_moves(O, s)
        took = legal[np.arange(B), a]
        valid += int(took.sum())
        idx = model_idx(moved[np.arange(B), a][took])
        for f in range(8):
            visited[f, idx[:, f]] = True
        loop_env.reset(done)
    P.sync(dev)
    assert torch.equal(env.boards, loop_env.boards) and torch.equal(env.aux, loop_env.aux)
    st = agent.stats()
    assert st["steps"] == B * steps and st["valid_moves"] == valid and st["explored"] == explored == valid
    v = agent.weights.cpu().numpy()
    assert np.isfinite(v).all() and np.abs(v).max() < 1e4
    changed = v != 0
    assert changed.any() and not (changed & ~visited).any(), "an entry no lane visited was written"
    assert changed.sum() > visited.sum() // 2 and agent.check_status() == 0


# ---------------------------------------------------------------------------------------------------------------
# 10. checkpoint
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_checkpoint_resumes_the_run(pkg, dev):
    """state_dict -> load_state_dict round-trips bit for bit, and 120 steps, a checkpoint, a fresh agent and env, 80
    more == 200 uninterrupted steps at B = 1 in all of V, boards, aux, statistics, counters and epsilon."""
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
    assert sd["kind"] == "line_afterstate" and sd["board_size"] == 4 and sd["weights"].device.type == "cpu"
    assert sd["weights"].dtype == torch.float32 and tuple(sd["weights"].shape) == (8, 65536)
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
    """Every other kind, shape and dtype is refused before anything is written, a line-tuple or row-tuple file cannot be
    promoted, and the three other agents refuse an afterstate checkpoint and keep their state."""
    env, agent = P.make_env(pkg, dev, 64), make_agent(pkg, dev)
    agent.fused_rollout(env, 20)
    good = agent.state_dict()
    before = P.learner_state(agent, env)
    rt, lt = P.make_agent(pkg, dev), LT.make_agent(pkg, dev)
    ht = pkg.BatchedQLearningAgent(10, capacity_log2=12, device="cpu", placement="plain")
    rt_sd, lt_sd = rt.state_dict(), lt.state_dict()
    marked = dict(good, weights=good["weights"] + 1.0, ctr=999, stats_i=good["stats_i"] + 1)
    wrong = [dict(marked, weights=marked["weights"].double()), dict(marked, weights=marked["weights"][:4]),
             dict(marked, weights=marked["weights"][:, :4096]), dict(marked, weights=marked["weights"].numpy()),
             dict(marked, weights=marked["weights"][:, :, None].expand(8, 65536, 4).contiguous()),
             dict(marked, board_size=5), dict(marked, stats_i=marked["stats_i"].int()),
             dict(marked, stats_f=marked["stats_f"][:2]), {k: v for k, v in marked.items() if k != "kind"},
             dict(marked, kind="row_tuple"), dict(marked, kind="line_tuple"), dict(rt_sd, ctr=999), dict(lt_sd, ctr=999),
             dict(lt_sd, kind="line_afterstate"), ht.state_dict()]
    for bad in wrong:
        with pytest.raises(ValueError):
            agent.load_state_dict(bad)
        P.sync(dev)
        P.assert_same_state(P.learner_state(agent, env), before)
    for bad in (rt_sd, lt_sd, marked):
        with pytest.raises(ValueError):
            agent.load_row_tuple(bad)
        P.sync(dev)
        P.assert_same_state(P.learner_state(agent, env), before)
    rt_before, lt_before = bits(rt.weights).copy(), bits(lt.weights).copy()
    with pytest.raises(ValueError):
        rt.load_state_dict(marked)
    with pytest.raises(ValueError, match="BatchedAfterstateAgent"):
        lt.load_state_dict(marked)
    with pytest.raises(ValueError):
        lt.load_row_tuple(marked)
    with pytest.raises(ValueError, match="BatchedAfterstateAgent"):
        ht.load_state_dict(good)
    assert np.array_equal(bits(rt.weights), rt_before) and np.array_equal(bits(lt.weights), lt_before)
    assert rt.ctr == 0 and lt.ctr == 0
    agent.load_state_dict(marked)
    assert agent.ctr == 999 and torch.equal(agent.weights.cpu(), marked["weights"])


@pytest.mark.parametrize("dev", DEVICES)
def test_python_surface(pkg, O, dev):
    """`values` is q2048_av_value, `q_values` the lookup, `update_q_value` ignores its reward argument (two calls that
    differ in it alone write the same bits), and the agent refuses a 5x5 env and an env profile."""
    agent, other = random_agent(pkg, dev, lr=0.1), random_agent(pkg, dev, lr=0.1)
    boards = midgame(O)[0][:300]
    tb = t8(dev, boards)
    q, legal, moved = model_eval(O, base_values(), boards, tuple(m[:300] for m in midgame(O)[1]))
    assert_same_bits(agent.values(tb), model_v(base_values(), boards), "values")
    assert_same_bits(agent.q_values(tb), q, "q_values")
    a = model_greedy(q, legal).astype(np.uint8)
    s2 = np.stack([spawned(np.random.default_rng(i), moved[i, a[i]]) for i in range(300)])
    done = np.zeros(300, np.uint8)
    agent.update_q_value(tb, a, np.zeros(300, F32), t8(dev, s2), done)
    other.update_q_value(tb, a, np.full(300, 1e6, F32), t8(dev, s2), done)
    assert agent.check_status() == 0
    if dev == "cpu":      # one thread per lane range on the twin too, but 300 lanes are one range: no race
        assert_same_bits(agent.weights, other.weights, "the reward entered the step")
    assert (bits(agent.weights) != bits(base_values())).any()
    with pytest.raises(ValueError):
        agent.update_q_value(tb, a, np.zeros(299, F32), t8(dev, s2), done)
    with pytest.raises(ValueError):
        agent.fused_rollout(pkg.BatchedGame2048Env(8, 5, dev, agent.seed, agent.env_id0), 1)
    with pytest.raises(ValueError):
        agent.fused_rollout(P.make_env(pkg, dev, 8, "nopenalty"), 1)
