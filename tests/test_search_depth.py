"""Two-level expectimax for the two afterstate families: q2048_{av,nt}_search_lookup_depth and
q2048_{av,nt}_search_play_rollout_depth against a numpy model, and the agents' `search_lookup(depth=)` /
`search_rollout(depth=)`.  (The scripts: test_search_depth_scripts.py.)

Which test executes which kernel (device) / function (CPU twin):
  k_search2_lookup<AvEvalOf|NtEvalOf>   test_crafted_boards, test_depths_disagree, test_batch_edges, test_device_equals_twin,
                                    test_python_surface
  k_search2_play_rollout<AvEvalOf|NtEvalOf, E>   test_player_against_the_model (E = 0..3 on the afterstate family, 0 and
                                    1 on the network), test_player_device_equals_twin, test_python_surface
  k_search_play_rollout<EVAL, E> and k_search2_play_rollout<EVAL, E>, EVAL = AvEvalOf, NtEvalOf, NtsEvalOf, E = 0..3
                                    test_searched_player_equals_the_four_call_loop
  depth 1 through the new entries   test_depth_one_is_the_existing_lookup, test_depth_one_is_the_existing_player
  the argument checks               test_abi, test_argument_errors_need_no_device, test_refused_calls_write_nothing

The model is numpy, composed from test_search's: best_1(nodes) = model_best(model_search(nodes).Q, legal) -- the
one-level model's searched row of every level-one node, and the first maximum over its legal moves -- fed to the same
literal formula (t_j = 9.0 * b2_j + b4_j in float64, the S_a sum as a Python loop in ascending j, one float64 division,
one rounding to float32, one float32 addition).  It shares no code with csrc/.  A level-one node's best_1 is remembered
by its 16 bytes (per family): the player's games revisit the boards that follow a reset.  Every comparison of a row, a
mask, a board, an aux record or an integer statistic is exact (float32 values as bit patterns), with canaries behind
every output; the base weights are asserted unwritten.

Every case runs on the CPU twin ("cpu") and on the GPU; the model's answers are computed once and shared."""
import os

import numpy as np
import pytest
import torch

import test_afterstate as AV
import test_ntuple as NT
import test_row_tuple_kernels as K
import test_row_tuple_player as P
import test_search as S

REPO = P.REPO
DEVICES = NT.DEVICES
FAMILIES = S.FAMILIES
ROOM, Q_CANARY, A_CANARY = K.ROOM, K.Q_CANARY, K.A_CANARY
ERR_NULL, ERR_SIZE, ERR_ALIGN, ERR_RANGE, ERR_FLAGS = -1, -2, -3, -6, -7
F32 = np.float32
EDGES = [1, 3, 4, 5, 63, 64, 65, 257]                   # the ends of a block and of a wave under either mapping
BAD_DEPTHS = (0, 3, -1)
NAMES = ("q2048_av_search_lookup_depth", "q2048_av_search_play_rollout_depth", "q2048_nt_search_lookup_depth",
         "q2048_nt_search_play_rollout_depth")
lib, t8, bits = K.lib, K.t8, K.bits
model_moves, model_best, mask_of, assert_same_bits = AV.model_moves, AV.model_best, AV.mask_of, NT.assert_same_bits
base_on, assert_base_unwritten, random_agent = S.base_on, S.assert_base_unwritten, S.random_agent
_SHARED = {}
_BEST1 = {"av": {}, "nt": {}}                            # level-one node (16 bytes) -> best_1, per family
CHUNK = 1024                                             # level-one nodes per call of the one-level model


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def best_1(O, fam, nodes):
    """best_1 of a batch of states: the one-level model's searched row of each, at the first maximum over its legal
    moves; 0.0f for a state without a legal move -> float32 [len(nodes)]"""
    memo, out = _BEST1[fam], np.zeros(len(nodes), F32)
    keys = [n.tobytes() for n in nodes]
    new = sorted({k for k in keys if k not in memo})
    for lo in range(0, len(new), CHUNK):
        part = new[lo:lo + CHUNK]
        q, legal, _ = S.model_search(O, fam, np.frombuffer(b"".join(part), np.uint8).reshape(-1, 16))
        b = model_best(q, legal)
        assert b.dtype == F32
        memo.update(zip(part, b))
    for i, k in enumerate(keys):
        out[i] = memo[k]
    return out


def model_search2(O, fam, boards):
    """The depth-2 row, by the definition -> (Q float32 [B, 4], legal bool [B, 4], level-one nodes, their best_1)"""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 16)
    moved, score, legal = model_moves(O, boards)
    nodes = S.model_nodes(moved, legal)
    best = best_1(O, fam, nodes)
    q, k = np.zeros((len(boards), 4), F32), 0
    for i in range(len(boards)):
        for a in range(4):
            if not legal[i, a]:
                continue                                                # Q_a = 0.0f, nothing evaluated
            n = int((moved[i, a] == 0).sum())
            assert 1 <= n <= 15
            s = 0.0
            for _ in range(n):                                          # ascending j, exactly this order
                t = 9.0 * float(best[k]) + float(best[k + 1])
                s = s + t
                k += 2
            e = F32(s / float(10 * n))                                  # one division, one rounding
            q[i, a] = F32(score[i, a]) + e
    assert k == len(best) and q.dtype == F32
    return q, legal, nodes, best


def lookup(L, fam, dev, boards, depth, name="search_lookup_depth"):
    """q2048_<fam>_search_lookup_depth (or, name="search_lookup", the entry without a depth) into canaried buffers
    -> (row bit patterns uint32 [B, 4], legal uint8 [B])"""
    B = len(boards)
    q = torch.full((B + ROOM, 4), Q_CANARY - (1 << 32), dtype=torch.int32, device=dev)
    legal = torch.full((B + ROOM,), A_CANARY, dtype=torch.uint8, device=dev)
    tb = t8(dev, boards)
    fn = getattr(L, f"q2048_{fam}_{name}")
    extra = () if depth is None else (depth,)
    assert fn(base_on(fam, dev).data_ptr(), tb.data_ptr(), B, *extra, q.data_ptr(), legal.data_ptr(), None) == 0
    P.sync(dev)
    q, legal = q.cpu().numpy().view(np.uint32), legal.cpu().numpy()
    assert (q[B:] == Q_CANARY).all() and (legal[B:] == A_CANARY).all(), "written beyond B"
    assert np.array_equal(tb.cpu().numpy(), np.asarray(boards, dtype=np.uint8)), "the boards were written"
    return q[:B], legal[:B]


def assert_rows2(L, O, fam, dev, boards, what):
    want, wlegal, nodes, best = model_search2(O, fam, boards)
    got, legal = lookup(L, fam, dev, boards, 2)
    assert_same_bits(got.view(F32), want, what)
    assert np.array_equal(legal, mask_of(wlegal)), what
    return want, wlegal, nodes, best


# ---------------------------------------------------------------------------------------------------------------
# 1. ABI and refusals
# ---------------------------------------------------------------------------------------------------------------
def test_abi(pkg):
    N = pkg._native
    with open(os.path.join(REPO, "include", "q2048.h")) as fh:
        header = fh.read()
    for name in NAMES:
        assert name in N._SIGNATURES, name
        assert hasattr(N.host_lib(), name) and hasattr(N.lib(), name), name
        assert f"int {name}(" in header, name
    for what in ("search_lookup", "search_play_rollout"):
        plain, deep = N._SIGNATURES[f"q2048_nt_{what}"], N._SIGNATURES[f"q2048_nt_{what}_depth"]
        assert N._SIGNATURES[f"q2048_av_{what}_depth"] == deep
        at = 3 if what == "search_lookup" else 5                      # `depth` after B / after steps
        assert deep[0] is plain[0] and deep[1][:at] + deep[1][at + 1:] == plain[1] and deep[1][at] is N.C.c_int
    for L in (N.host_lib(), N.lib()):
        assert b"depth" in L.q2048_strerror(ERR_RANGE)
    assert N.host_lib().q2048_abi_version() == N.lib().q2048_abi_version() == N.ABI_VERSION


def with_depth(fn, depth, at):
    return lambda *a: fn(*a[:at], depth, *a[at:])


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("which", ["hip", "host"])
def test_argument_errors_need_no_device(pkg, which, fam):
    """A depth of 0, 3 or -1 is Q2048_ERR_RANGE ahead of a NULL pointer, a negative B and a misaligned pointer (each of
    which alone has another code).  With depth 1 and 2 the counterpart's checks follow in its order -- the lookup's B,
    NULL, alignment; the player's B, flags, NULL, alignment, steps, eps -- on both libraries with made-up addresses,
    and B == 0 / steps == 0 are no-ops."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    look, play = getattr(L, f"q2048_{fam}_search_lookup_depth"), getattr(L, f"q2048_{fam}_search_play_rollout_depth")
    good = [0x1000, 0x2000, 64, 0x3000, 0x4000, None]                    # (without the depth)
    pointers, aligned, big = (0, 1, 3, 4), (0, 1, 3), (2 ** 31 - 1) * 256 + 1
    for depth in BAD_DEPTHS:
        f = with_depth(look, depth, 3)
        assert f(*good) == ERR_RANGE and f(None, 0x2000, 64, 0x3000, 0x4000, None) == ERR_RANGE
        assert f(0x1000, 0x2000, -1, 0x3000, 0x4000, None) == ERR_RANGE and f(0x1008, 0x2000, 64, 0x3000, 0x4000, None) == ERR_RANGE
        assert f(None, 0x2008, -1, 0x3008, None, None) == ERR_RANGE and f(0x1000, 0x2000, 0, 0x3000, 0x4000, None) == ERR_RANGE
        g = with_depth(play, depth, 5)
        ok = [0x1000, 0x2000, 0x3000, 64, 1, 0.0, 1, 0, 0, 0, None, None, 0x4000, None]
        bad = lambda **kw: g(*[kw.get(str(i), v) for i, v in enumerate(ok)])   # noqa: E731
        assert bad() == ERR_RANGE and bad(**{"0": None}) == ERR_RANGE and bad(**{"3": -1}) == ERR_RANGE
        assert bad(**{"2": 0x3008}) == ERR_RANGE and bad(**{"9": 64}) == ERR_RANGE and bad(**{"4": -1}) == ERR_RANGE
        assert bad(**{"5": 2.0}) == ERR_RANGE and bad(**{"3": 0}) == ERR_RANGE and bad(**{"4": 0}) == ERR_RANGE
    for depth in (1, 2):
        fn = with_depth(look, depth, 3)

        def call(**kw):
            args = list(good)
            for pos, value in kw.items():
                args[int(pos[1:])] = value
            return fn(*args)

        bad_align = {f"p{pos}": good[pos] + 8 for pos in aligned}
        for value in (-1, big):
            assert call(p2=value, p0=None, p3=good[3] + 8) == ERR_SIZE
        for pos in pointers:
            assert call(**{**bad_align, f"p{pos}": None}) == ERR_NULL, f"NULL in position {pos}"
        for pos in aligned:
            assert call(**{f"p{pos}": good[pos] + 8}) == ERR_ALIGN, f"position {pos} off by 8 bytes"
        assert call(p2=0) == 0 and call(p2=0, p4=None) == ERR_NULL and call(p2=0, p3=good[3] + 8) == ERR_ALIGN
        ok = P.argument_errors(with_depth(play, depth, 5), 0x1000, 0x2000, 0x3000, 0x4000)
        for bit in (N.FLAG_INDEPENDENT, N.FLAG_SYMMETRIC, N.FLAG_SINGLE_ENV, N.FLAG_TD_CAS, N.FLAG_PLAY_ONLY, N.FLAG_NO_LEARN,
                    N.FLAG_NO_NEW_ROWS, N.FLAG_LINE_SUMMARY, 1 << 8, 1 << 23, 1 << 30, 1 << 31):
            assert ok(flags=bit) == ERR_FLAGS and ok(flags=bit | N.FLAG_ENV_DQN | N.FLAG_RESET_SHAPING) == ERR_FLAGS, bit
        assert ok(B=0) == 0 and ok(steps=0) == 0
        assert ok(B=0, boards=None) == ERR_NULL and ok(steps=0, weights=0x3008) == ERR_ALIGN
        assert ok(B=0, flags=N.FLAG_INDEPENDENT) == ERR_FLAGS


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
def test_refused_calls_write_nothing(pkg, dev, fam):
    """Both entry points refused for the depth with everything else in order, and, at depth 2, for their LAST check on
    real buffers (and the lookup once for a missing legal_out): the weights, boards, aux, both outputs, both
    statistics vectors and status keep every byte."""
    L, B, nan = lib(pkg, dev), 64, float("nan")
    V = base_on(fam, dev)
    boards = t8(dev, K.random_boards(np.random.default_rng(1), B))
    aux = torch.full((B, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    q_out = torch.full((B * 4 + 8,), 0x6B6B6B6B, dtype=torch.int32, device=dev)
    legal_out = torch.full((B + 8,), A_CANARY, dtype=torch.uint8, device=dev)
    si, sf = torch.full((64,), 7, dtype=torch.int64, device=dev), torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((1,), 0x777, dtype=torch.int32, device=dev)
    everything = (boards, aux, q_out, legal_out, si, sf, status)
    before = [t.clone() for t in everything]
    p = lambda t: t.data_ptr()      # noqa: E731
    look, play = getattr(L, f"q2048_{fam}_search_lookup_depth"), getattr(L, f"q2048_{fam}_search_play_rollout_depth")
    calls = [look(p(V), p(boards), B, d, p(q_out), p(legal_out), None) for d in BAD_DEPTHS]
    calls += [play(p(boards), p(aux), p(V), B, 3, d, 0.0, 1, 0, 0, 0, p(si), p(sf), p(status), None) for d in BAD_DEPTHS]
    calls += [
        look(p(V), p(boards), B, 2, p(q_out) + 8, p(legal_out), None),
        look(p(V), p(boards), B, 2, p(q_out), None, None),
        look(p(V), p(boards), -1, 2, p(q_out), p(legal_out), None),
        play(p(boards), p(aux), p(V), B, 3, 2, nan, 1, 0, 0, 0, p(si), p(sf), p(status), None),
        play(p(boards), p(aux), p(V), B, 3, 2, 0.0, 1, 0, 0, 1 << 8, p(si), p(sf), p(status), None),
        play(p(boards), p(aux), p(V), B, -1, 2, 0.0, 1, 0, 0, 0, p(si), p(sf), p(status), None),
    ]
    P.sync(dev)
    assert calls == [ERR_RANGE] * 6 + [ERR_ALIGN, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_FLAGS, ERR_SIZE]
    for t, b in zip(everything, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "a refused call wrote"
    assert_base_unwritten(fam, dev, "a refused call wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 2. depth 1 is the existing entry points
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
def test_depth_one_is_the_existing_lookup(pkg, dev, fam):
    rng = np.random.default_rng(257)
    boards = K.random_boards(rng, 257)
    boards[rng.random(boards.shape) < 0.33] = 0
    L = lib(pkg, dev)
    old, old_mask = lookup(L, fam, dev, boards, None, "search_lookup")
    new, new_mask = lookup(L, fam, dev, boards, 1)
    assert np.array_equal(old, new) and np.array_equal(old_mask, new_mask) and len(set(new_mask.tolist())) > 4
    assert_base_unwritten(fam, dev, "the lookup wrote the weights")


def play(L, fam, dev, env, steps, eps, depth, si, sf, status):
    """One launch of q2048_<fam>_search_play_rollout[_depth] on `env` (depth None: the entry without a depth)."""
    name = f"q2048_{fam}_search_play_rollout" + ("" if depth is None else "_depth")
    extra = () if depth is None else (depth,)
    code = getattr(L, name)(env.boards.data_ptr(), env.aux.data_ptr(), base_on(fam, dev).data_ptr(), env.num_envs, steps,
                            *extra, eps, env.seed, env.env_id0, env.ctr & 0xFFFFFFFF, env.env_flags, si.data_ptr(),
                            sf.data_ptr(), status.data_ptr(), None)
    assert code == 0
    env.ctr += steps


def played(pkg, fam, dev, sd, B, cuts, eps, depth, profile="shaped", rss=False):
    """The raw entry point from the state `sd` in launches of `cuts` -> (boards, aux bytes, integer statistics), canaried"""
    N = pkg._native
    env = S.env_from(pkg, dev, B, profile, rss, sd)
    si = torch.zeros(N.NSTAT_I + ROOM, dtype=torch.int64, device=dev)
    sf = torch.zeros(N.NSTAT_F + ROOM, dtype=torch.float64, device=dev)
    si[N.NSTAT_I:], sf[N.NSTAT_F:] = 0x5151, 5151.0
    status = torch.full((1,), 0x777, dtype=torch.int32, device=dev)
    for c in cuts:
        play(lib(pkg, dev), fam, dev, env, c, eps, depth, si, sf, status)
    P.sync(dev)
    assert (si[N.NSTAT_I:] == 0x5151).all() and (sf[N.NSTAT_F:] == 5151.0).all() and int(status.item()) == 0x777
    return env.boards.cpu(), env.aux.cpu().contiguous().view(torch.uint8), si[:N.NSTAT_I].cpu().numpy()


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
def test_depth_one_is_the_existing_player(pkg, dev, fam):
    N = pkg._native
    sd, _ = S.crowded_start(pkg, 65, "shaped", False)
    old, new = (played(pkg, fam, dev, sd, 65, (1, 15), 0.3, depth) for depth in (None, 1))
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1]), "boards or aux bytes differ"
    assert np.array_equal(old[2], new[2]) and new[2][N.ST_STEPS] == 65 * 16 and new[2][N.ST_EXPLORE] > 0
    assert_base_unwritten(fam, dev, "the player wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 3. crafted boards
# ---------------------------------------------------------------------------------------------------------------
# Moving left gives an afterstate with cells 14 and 15 empty; a 4 at cell 15 makes it test_search's ZERO_BEST: a level-one
# node that is alive (its own move left is legal) and whose chance node "left, a 2 at cell 15" is a full board without
# equal neighbours
DEAD_LEAF = np.array([3, 4, 3, 4, 4, 3, 4, 3, 3, 4, 3, 4, 0, 4, 3, 0], np.uint8)


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
def test_crafted_boards(pkg, O, dev, fam):
    L = lib(pkg, dev)
    boards = np.stack([S.lone_tile(0), S.lone_tile(5), S.lone_tile(15), S.ONE_PAIR, S.ONE_MOVE, P.DEAD.numpy(), S.ZERO_BEST,
                       DEAD_LEAF])
    want, legal, nodes, best = assert_rows2(L, O, fam, dev, boards, "crafted boards")
    per_board = [len(S.model_nodes(*[x[i:i + 1] for x in model_moves(O, boards)[::2]])) for i in range(len(boards))]
    assert per_board[:6] == [60, 120, 60, 4, 24, 0] and sum(per_board) == len(nodes)
    assert mask_of(legal)[:6].tolist() == [0b1100, 0b1111, 0b0011, 0b0101, 0b1000, 0]
    assert not bits(want[5]).any() and lookup(L, fam, dev, P.DEAD.numpy()[None], 2)[1][0] == 0, "no legal move: all +0.0, mask 0"
    assert (bits(want[:5]) != 0).sum() == 2 + 4 + 2 + 2 + 1, "an illegal move reads +0.0, a legal one its mean"
    # ZERO_BEST: its move left has ONE empty cell; the level-one node behind the 2 has no legal move, so a 0.0f best_1
    # enters the sum with nothing beneath it; the node behind the 4 is alive
    moved, score, zlegal = model_moves(O, S.ZERO_BEST[None])
    assert zlegal[0, 0] and int((moved[0, 0] == 0).sum()) == 1 and score[0, 0] == 0
    znodes = S.model_nodes(moved, zlegal & np.array([True, False, False, False]))
    nlegal = model_moves(O, znodes)[2]
    b2, b4 = best_1(O, fam, znodes)
    assert not nlegal[0].any() and bits(np.array([b2]))[0] == 0 and nlegal[1].any() and b4 != 0
    assert bits(want[6, :1])[0] == bits(np.array([F32((9.0 * 0.0 + float(b4)) / 10.0)]))[0], "a 0.0f best_1 enters the sum"
    # DEAD_LEAF: a level-one node that is alive with a chance node of its own that is dead
    moved, _, dlegal = model_moves(O, DEAD_LEAF[None])
    level_one = S.model_nodes(moved, dlegal)
    at = [i for i, n in enumerate(level_one) if np.array_equal(n, S.ZERO_BEST)]
    assert len(at) == 1 and model_moves(O, level_one[at])[2].any(), "the node is alive"
    m1, _, l1 = model_moves(O, level_one[at])
    leaves = S.model_nodes(m1, l1)
    assert (~model_moves(O, leaves)[2].any(axis=1)).sum() >= 1, "and one of its chance nodes is dead"
    # cells of 16 and 17
    al = S.aliased_boards(O)
    assert_rows2(L, O, fam, dev, al, "cells of 16 and 17")
    assert_base_unwritten(fam, dev, "the lookup wrote the weights")


def midgame_model2(O, fam):
    """test_search's 257 mid-game boards with the model's depth-2 rows beside its depth-1 rows, computed once."""
    key = ("mid2", fam)
    if key not in _SHARED:
        boards, q1, legal, _ = S.midgame_model(O, fam)
        q2, legal2, _, _ = model_search2(O, fam, boards)
        assert np.array_equal(legal, legal2)
        q2.setflags(write=False)
        _SHARED[key] = (boards, q1, q2, legal)
    return _SHARED[key]


# ---------------------------------------------------------------------------------------------------------------
# 4. the depths disagree
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
def test_depths_disagree(pkg, O, dev, fam):
    """Among the 257 mid-game boards the model selects those on which the depth-2 first maximum over the legal moves is
    another move than the depth-1 one; there are some, and on them the library's rows are the model's and pick its moves."""
    boards, q1, q2, legal = midgame_model2(O, fam)
    a1, a2 = AV.model_greedy(q1, legal), AV.model_greedy(q2, legal)
    pick = np.flatnonzero((a1 != a2) & legal.any(axis=1))
    assert 0 < len(pick) < len(boards)
    got, mask = lookup(lib(pkg, dev), fam, dev, boards[pick], 2)
    assert_same_bits(got.view(F32), q2[pick], "the boards on which the depths disagree")
    assert np.array_equal(mask, mask_of(legal[pick]))
    assert np.array_equal(AV.model_greedy(got.view(F32), legal[pick]), a2[pick])
    shallow, _ = lookup(lib(pkg, dev), fam, dev, boards[pick], 1)
    assert np.array_equal(AV.model_greedy(shallow.view(F32), legal[pick]), a1[pick])


# ---------------------------------------------------------------------------------------------------------------
# 5. batch edges, and 6. the device against the twin
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
def test_batch_edges(pkg, O, dev, fam, B):
    """The last B of the 257 mid-game boards (so that every B starts on another board): full rows and masks."""
    boards, _, q2, legal = midgame_model2(O, fam)
    got, mask = lookup(lib(pkg, dev), fam, dev, boards[-B:], 2)
    assert_same_bits(got.view(F32), q2[-B:], f"B = {B}")
    assert np.array_equal(mask, mask_of(legal[-B:]))
    assert_base_unwritten(fam, dev, "the lookup wrote the weights")


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES)
def test_device_equals_twin(pkg, fam):
    """1,024 random boards (cells 0..15, a third of them emptied), full rows and masks: the device's bits are the twin's."""
    rng = np.random.default_rng(1024)
    boards = K.random_boards(rng, 1024)
    boards[rng.random(boards.shape) < 0.33] = 0
    N = pkg._native
    host, hmask = lookup(N.host_lib(), fam, "cpu", boards, 2)
    got, mask = lookup(N.lib(), fam, "cuda:0", boards, 2)
    assert_same_bits(got.view(F32), host.view(F32), "device and twin")
    assert np.array_equal(mask, hmask) and len(set(mask.tolist())) > 4


# ---------------------------------------------------------------------------------------------------------------
# 7. the player
# ---------------------------------------------------------------------------------------------------------------
STEPS, CUTS = 24, (1, 7, 16)
PLAYER_CASES = [(fam, B, eps, profile, rss) for fam in FAMILIES for B in (3, 9) for eps in (0.0, 0.3)
                for profile, rss in (("shaped", False), ("shaped", True), ("nopenalty", False), ("nopenalty", True))
                if fam == "av" or not rss]


def model_play2(pkg, O, fam, B, eps, profile, rss):
    """test_search.model_play with the depth-2 row: the player's draw contract, the env's four-call step and reset on
    the CPU twin with the same draws, once per case.
    -> (start state, boards, aux, ctr, integer statistics, {float statistic: its terms}, boards of the DEPTH-1 player)"""
    key = ("play2", fam, B, eps, profile, rss)
    if key in _SHARED:
        return _SHARED[key]
    N = pkg._native
    sd, dead = S.crowded_start(pkg, B, profile, rss)
    model = S.env_from(pkg, "cpu", B, profile, rss, sd)
    si = np.zeros(N.NSTAT_I, np.int64)
    terms = {N.SF_RETURN: [], N.SF_RETURN_SQ: [], N.SF_REWARD: []}
    for _ in range(STEPS):
        q, legal, _, _ = model_search2(O, fam, model.boards.numpy())
        acts, explored = P.model_actions(O, q, mask_of(legal), model.seed, model.env_id0, model.ctr, eps)
        _, reward, done, _ = model.step(torch.from_numpy(acts))
        d = done.numpy().astype(bool)
        f = model.aux_fields()
        si[N.ST_STEPS] += B
        si[N.ST_VALID] += int(legal.any(axis=1).sum())
        si[N.ST_EXPLORE] += explored
        si[N.ST_EPISODES] += int(d.sum())
        si[N.ST_SCORE] += int(f["score"][d].astype(np.int64).sum())
        for m in model.max_log2.numpy()[d]:
            si[N.ST_HIST0 + min(int(m), 22)] += 1
        ret = f["ep_return"][d].astype(np.float64)
        terms[N.SF_RETURN] += ret.tolist()
        terms[N.SF_RETURN_SQ] += (ret * ret).tolist()
        terms[N.SF_REWARD] += reward.numpy().astype(np.float64).tolist()
        model.reset(done)
    assert si[N.ST_EPISODES] >= dead > 0, "the span must cover the reset path"
    shallow_env = S.env_from(pkg, "cpu", B, profile, rss, sd)
    random_agent(pkg, fam, "cpu").search_rollout(shallow_env, STEPS, epsilon=eps)
    _SHARED[key] = (sd, model.boards.clone(), model.aux.clone(), model.ctr, si, terms, shallow_env.boards.clone())
    return _SHARED[key]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("fam,B,eps,profile,rss", PLAYER_CASES)
def test_player_against_the_model(pkg, O, dev, fam, B, eps, profile, rss):
    """24 steps in launches of 1 + 7 + 16 from crowded boards with dead boards in front: boards, aux bytes, env.ctr, the
    integer statistics vector and the float64 one against the model loop; the weights, the training statistics and
    `status` are not written; episodes end inside the span; and at epsilon 0 the depth-1 player, started from the same
    bytes, ends on other boards -- the row handed to the choice really is the depth-2 one."""
    N = pkg._native
    sd, boards, aux, ctr, si, terms, shallow_boards = model_play2(pkg, O, fam, B, eps, profile, rss)
    env = S.env_from(pkg, dev, B, profile, rss, sd)
    agent = random_agent(pkg, fam, dev)
    agent.status.fill_(0x777)
    train_stats = agent.stats_i.clone(), agent.stats_f.clone()
    for c in CUTS:
        agent.search_rollout(env, c, epsilon=eps, depth=2)
    P.sync(dev)
    assert torch.equal(env.boards.cpu(), boards), "boards differ"
    assert torch.equal(env.aux.cpu(), aux), "aux records differ"
    assert env.ctr == ctr == P.WARM + STEPS
    got_i, got_f = (t.cpu().numpy() for t in agent._play_stats)
    assert np.array_equal(got_i, si), f"integer statistics: {got_i.tolist()} != {si.tolist()}"
    assert si[N.ST_STEPS] == B * STEPS and si[N.ST_EPISODES] > 0
    for k in range(N.NSTAT_F):
        S.assert_order_free_sum(float(got_f[k]), terms.get(k, []), f"float statistic {k}")
    if eps == 0.0:
        assert si[N.ST_EXPLORE] == 0
        assert not torch.equal(boards, shallow_boards), "the depth-2 player played the depth-1 player's games"
    else:
        assert 0 < si[N.ST_EXPLORE] < 0.6 * B * STEPS
    assert_base_unwritten(fam, dev, "the player wrote to the weights")
    assert torch.equal(agent.stats_i, train_stats[0]) and torch.equal(agent.stats_f, train_stats[1])
    assert int(agent.status.item()) == 0x777, "status: required, never written"


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("profile,rss", [("shaped", False), ("nopenalty", True)])
def test_player_device_equals_twin(pkg, fam, profile, rss):
    """B = 257 over 8 steps in launches of 1 + 7 at epsilon 0.3, byte for byte: the ends of a block and of a wave
    without the numpy cost."""
    N = pkg._native
    sd, _ = S.crowded_start(pkg, 257, profile, rss)
    host, dev = (played(pkg, fam, d, sd, 257, (1, 7), 0.3, 2, profile, rss) for d in ("cpu", "cuda:0"))
    assert torch.equal(host[0], dev[0]) and torch.equal(host[1], dev[1]), "boards or aux bytes differ"
    assert np.array_equal(host[2], dev[2]) and dev[2][N.ST_STEPS] == 257 * 8 and dev[2][N.ST_EPISODES] > 0


# ---------------------------------------------------------------------------------------------------------------
# 8. the Python surface
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
def test_python_surface(pkg, O, dev, fam, monkeypatch):
    """`search_lookup(depth=2)` and `search_rollout(depth=2)` reach the new entry points (and depth 1 the old ones, as
    before); a depth of 3 raises ValueError before any native call."""
    boards, q1, q2, legal = midgame_model2(O, fam)
    agent = random_agent(pkg, fam, dev)
    calls, real = [], agent._fn
    monkeypatch.setattr(agent, "_fn", lambda name: calls.append(name) or real(name))
    got, mask = agent.search_lookup(t8(dev, boards[:33]), depth=2)
    assert got.dtype == torch.float32 and tuple(got.shape) == (33, 4) and got.device == agent.device
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (33,) and mask.device == agent.device
    assert_same_bits(got, q2[:33], "search_lookup(depth=2)")
    assert np.array_equal(mask.cpu().numpy(), mask_of(legal[:33]))
    assert_same_bits(agent.search_lookup(t8(dev, boards[:33]))[0], q1[:33], "search_lookup()")
    assert_same_bits(agent.search_lookup(t8(dev, boards[:33]), depth=1)[0], q1[:33], "search_lookup(depth=1)")
    env = P.make_env(pkg, dev, 9)
    agent.search_rollout(env, 3, depth=2)
    agent.search_rollout(env, 2, epsilon=1.0, depth=2)
    agent.search_rollout(env, 1)
    P.sync(dev)
    assert calls == ["search_lookup_depth", "search_lookup", "search_lookup", "search_play_rollout_depth",
                     "search_play_rollout_depth", "search_play_rollout"]
    st = agent.play_stats()
    assert env.ctr == 6 and st["steps"] == 54 and st["explored"] == 18 and st["valid_moves"] == 54
    assert agent.stats()["steps"] == 0, "the training statistics never see the player"
    for bad in (3, 0, -1, True, 2.5, None):
        with pytest.raises(ValueError, match="depth"):
            agent.search_lookup(t8(dev, boards[:4]), depth=bad)
        with pytest.raises(ValueError, match="depth"):
            agent.search_rollout(env, 1, depth=bad)
    assert len(calls) == 6 and env.ctr == 6 and agent.play_stats()["steps"] == 54
    with pytest.raises(ValueError):
        agent.search_rollout(pkg.BatchedGame2048Env(8, 5, dev, agent.seed, agent.env_id0), 1, depth=2)
    assert_base_unwritten(fam, dev, "the surface wrote to the weights")


# ---------------------------------------------------------------------------------------------------------------
# 9. every searched player, every env profile: the rollout against the four-call loop
# ---------------------------------------------------------------------------------------------------------------
LOOP_B, STAGE_TILES = 5, (32, 128)
LOOP_CASES = [(fam, depth, profile, rss) for fam in ("av", "nt", "nts") for depth in (1, 2)
              for profile, rss in (("shaped", False), ("shaped", True), ("nopenalty", False), ("nopenalty", True))]


class SearchedRows:
    """What P.four_call_loop asks of an agent, with the searched row as the row: q_values = search_lookup(depth)[0]."""

    def __init__(self, agent, depth):
        self.agent, self.depth = agent, depth

    def q_values(self, boards):
        return self.agent.search_lookup(boards, depth=self.depth)[0]

    def stats(self):
        return self.agent.stats()


def searched_agent(pkg, fam, dev):
    """-> (agent on weights that are only read, the assertion that they still are).  "nts": the staged network with
    tiles (32, 128) on test_ntuple_stages' three tables (that module imports this one, hence the import here)."""
    if fam != "nts":
        return random_agent(pkg, fam, dev), lambda what: assert_base_unwritten(fam, dev, what)
    import test_ntuple_stages as ST
    agent = ST.make_agent(pkg, dev, STAGE_TILES, weights=ST.tables_on(dev, 3))
    return agent, lambda what: ST.assert_tables_unwritten(dev, 3, what)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("fam,depth,profile,rss", LOOP_CASES)
def test_searched_player_equals_the_four_call_loop(pkg, dev, fam, depth, profile, rss):
    """B = 5 crowded boards (one dead board in front; a second block with one live wave at depth 1, five blocks at
    depth 2), epsilon 0, 24 steps by search_rollout in launches of 1 + 7 + 16 and by the four-call loop on a twin env:
    the search LOOKUP for the row, q2048_legal_moves, the env's own step and reset -- no player kernel.  Both families
    and the staged network, both depths, all four env profiles: boards, aux, the statistics; nothing explored; the
    weights are not written."""
    start, dead = AV.midgame_env(pkg, "cpu", LOOP_B, profile, rss, dead=1)
    env = S.env_from(pkg, dev, LOOP_B, profile, rss, start.state_dict())
    env_loop = P.twin_of(pkg, env)
    agent, assert_unwritten = searched_agent(pkg, fam, dev)
    for c in CUTS:
        agent.search_rollout(env, c, depth=depth)
    st_loop = P.four_call_loop(SearchedRows(agent, depth), env_loop, STEPS)
    P.sync(dev)
    st = agent.play_stats()
    assert torch.equal(env.boards, env_loop.boards), "boards differ"
    assert torch.equal(env.aux, env_loop.aux), "aux records differ"
    assert env.ctr == env_loop.ctr == P.WARM + STEPS
    assert st["steps"] == st_loop["steps"] == LOOP_B * STEPS and st["valid_moves"] == st_loop["valid_moves"]
    assert st["episodes"] == st_loop["episodes"] >= dead == 1, "the span must cover the reset path"
    assert st["max_tile_hist"] == st_loop["max_tile_hist"]
    assert st["explored"] == 0
    assert_unwritten("the player wrote to the weights")
