"""One-level expectimax over the spawn for the two afterstate families: q2048_{av,nt}_search_lookup and
q2048_{av,nt}_search_play_rollout against a numpy model, and the agents' `search_lookup` / `search_rollout`.
(The scripts: test_search_scripts.py.)

Which test executes which kernel (device) / function (CPU twin):
  k_search_lookup<AvEvalOf|NtEvalOf>   test_crafted_boards, test_searched_and_greedy_choices_differ, test_batch_edges,
                                    test_device_equals_twin, test_python_surface
  k_search_play_rollout<AvEvalOf|NtEvalOf, E>   test_player_against_the_model (E = 0..3 on the afterstate family, 0 and
                                    1 on the network), test_python_surface; E = 0..3 on both:
                                    test_search_depth.test_searched_player_equals_the_four_call_loop
  the argument checks               test_abi, test_argument_errors_need_no_device, test_refused_calls_write_nothing

The model (model_search) is plain numpy: the afterstates come from the oracle's move (test_afterstate.model_moves), the
chance nodes are built cell by cell, evaluated with the families' existing models (test_afterstate.model_eval,
test_ntuple.model_eval, model_best) and combined by the definition taken literally: t_j = 9.0 * b2_j + b4_j in float64,
the S_a sum as a Python loop in ascending j, one float64 division, one rounding to float32, one float32 addition.  It
shares no code with csrc/.  Every comparison of a row, a mask, a board, an aux record or an integer statistic is exact
(float32 values as bit patterns), with canaries behind every output.

Two things differ from a naive reading of the case list, both asserted where they matter:
  * a lone tile in a CORNER (cell 0, cell 15) has two legal moves, not four: it cannot move towards its own corner.
    Cell 5 has four legal moves and 15 empty cells each: all 120 node slots.  And on a FULL board a move is legal iff
    its opposite is (a line with an equal pair merges both ways), so one merging pair gives 2 legal moves and 4 nodes;
    the board with exactly ONE legal move is a full row against its wall.
  * the env model of the player test is the batched env's own four-call step on the CPU twin (what the player tests of
    the other families use): the oracle's shaped reward agrees with float32 only to 1 ulp (test_gpu_parity), so it
    cannot give aux bytes.  The float64 statistics are sums that the device accumulates with atomics in an unspecified
    order; `assert_order_free_sum` compares them exactly where every order gives the same double and otherwise within
    the rounding of the additions themselves.

Every case runs on the CPU twin ("cpu") and on the GPU; the model's answers are computed once and shared."""
import os
import types

import numpy as np
import pytest
import torch

import test_afterstate as AV
import test_ntuple as NT
import test_row_tuple_kernels as K
import test_row_tuple_player as P

REPO = P.REPO
DEVICES = NT.DEVICES
FAMILIES = ["av", "nt"]
ROOM, Q_CANARY, A_CANARY = K.ROOM, K.Q_CANARY, K.A_CANARY
ERR_NULL, ERR_SIZE, ERR_ALIGN, ERR_RANGE, ERR_FLAGS = -1, -2, -3, -6, -7
F32 = np.float32
EDGES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257]         # the ends of a block of four boards, of a wave and of 256 lanes
NAMES = ("q2048_av_search_lookup", "q2048_av_search_play_rollout", "q2048_nt_search_lookup", "q2048_nt_search_play_rollout")
lib, t8, t32, bits = K.lib, K.t8, K.t32, K.bits
model_moves, model_best, mask_of, assert_same_bits = AV.model_moves, AV.model_best, AV.mask_of, NT.assert_same_bits
_SHARED = {}


# ---------------------------------------------------------------------------------------------------------------
# the two families: their values, their model of one evaluation, their agent
# ---------------------------------------------------------------------------------------------------------------
def base_values(fam):
    return AV.base_values() if fam == "av" else NT.base_values()


def base_on(fam, dev):
    """The family's random values on `dev`, uploaded once (the network's 256 MiB are test_ntuple's copy); only read."""
    if fam == "nt":
        return NT.base_on(dev)
    key = ("av", str(dev))
    if key not in _SHARED:
        _SHARED[key] = t32(dev, AV.base_values())
    return _SHARED[key]


def assert_base_unwritten(fam, dev, what):
    assert np.array_equal(bits(base_on(fam, dev)), bits(base_values(fam))), what


def model_eval(O, fam, boards):
    return (AV if fam == "av" else NT).model_eval(O, base_values(fam), boards)


def random_agent(pkg, fam, dev, **kw):
    agent = (AV if fam == "av" else NT).make_agent(pkg, dev, **kw)
    agent.weights = base_on(fam, dev)           # only read by what follows; each test asserts so
    return agent


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def model_nodes(moved, legal):
    """The chance nodes of a batch in slot order: for every board, legal move a, empty cell j of c_a (ascending) the
    board with a 2 at j, then the board with a 4 at j -> uint8 [nodes, 16]"""
    nodes = []
    for i in range(len(moved)):
        for a in range(4):
            if legal[i, a]:
                for j in np.flatnonzero(moved[i, a] == 0):
                    for tile in (1, 2):
                        node = moved[i, a].copy()
                        node[j] = tile
                        nodes.append(node)
    return np.array(nodes, dtype=np.uint8).reshape(-1, 16)


def model_search(O, fam, boards):
    """The searched row, by the definition -> (Q float32 [B, 4], legal bool [B, 4], best of every node float32 [nodes])"""
    boards = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 16)
    moved, score, legal = model_moves(O, boards)
    nodes = model_nodes(moved, legal)
    best = np.zeros(0, F32)
    if len(nodes):
        nq, nlegal, _ = model_eval(O, fam, nodes)
        best = model_best(nq, nlegal)
        assert best.dtype == F32
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
    return q, legal, best


def search_lookup(L, fam, dev, boards):
    """q2048_<fam>_search_lookup into canaried buffers -> (row bit patterns uint32 [B, 4], legal uint8 [B])"""
    B = len(boards)
    q = torch.full((B + ROOM, 4), Q_CANARY - (1 << 32), dtype=torch.int32, device=dev)
    legal = torch.full((B + ROOM,), A_CANARY, dtype=torch.uint8, device=dev)
    tb = t8(dev, boards)
    fn = getattr(L, f"q2048_{fam}_search_lookup")
    assert fn(base_on(fam, dev).data_ptr(), tb.data_ptr(), B, q.data_ptr(), legal.data_ptr(), None) == 0
    P.sync(dev)
    q, legal = q.cpu().numpy().view(np.uint32), legal.cpu().numpy()
    assert (q[B:] == Q_CANARY).all() and (legal[B:] == A_CANARY).all(), "written beyond B"
    assert np.array_equal(tb.cpu().numpy(), np.asarray(boards, dtype=np.uint8)), "the boards were written"
    return q[:B], legal[:B]


def assert_rows(L, O, fam, dev, boards, what):
    want, wlegal, best = model_search(O, fam, boards)
    got, legal = search_lookup(L, fam, dev, boards)
    assert_same_bits(got.view(F32), want, what)
    assert np.array_equal(legal, mask_of(wlegal)), what
    return want, wlegal, best


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
    for what in ("search_lookup", "search_play_rollout"):
        assert N._SIGNATURES[f"q2048_av_{what}"] == N._SIGNATURES[f"q2048_nt_{what}"]
    assert N._SIGNATURES["q2048_nt_search_play_rollout"] == N._SIGNATURES["q2048_nt_play_rollout"]
    assert N.host_lib().q2048_abi_version() == 7 == N.lib().q2048_abi_version() == N.ABI_VERSION
    assert "#define Q2048_ABI_VERSION 7 " in header
    for cls in (pkg.BatchedAfterstateAgent, pkg.BatchedNTupleAgent):
        assert callable(cls.search_lookup) and callable(cls.search_rollout)
    assert pkg.BatchedNTupleAgent.search_rollout is pkg.BatchedAfterstateAgent.search_rollout   # inherited through _FAMILY


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("which", ["hip", "host"])
def test_argument_errors_need_no_device(pkg, which, fam):
    """The order of q2048_{av,nt}_lookup -- B, NULL, alignment -- with `legal_out` one more required pointer, and the
    order of q2048_{av,nt}_play_rollout -- B, flags, NULL, alignment, steps, eps -- on both libraries with made-up
    addresses: every refused call also carries the errors that come later, and B == 0 / steps == 0 are no-ops."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    fn = getattr(L, f"q2048_{fam}_search_lookup")
    good = [0x1000, 0x2000, 64, 0x3000, 0x4000, None]
    pointers, aligned, big = (0, 1, 3, 4), (0, 1, 3), (2 ** 31 - 1) * 256 + 1

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
    ok = P.argument_errors(getattr(L, f"q2048_{fam}_search_play_rollout"), 0x1000, 0x2000, 0x3000, 0x4000)
    for bit in (N.FLAG_INDEPENDENT, N.FLAG_SYMMETRIC, N.FLAG_SINGLE_ENV, N.FLAG_TD_CAS, N.FLAG_PLAY_ONLY, N.FLAG_NO_LEARN,
                N.FLAG_NO_NEW_ROWS, N.FLAG_LINE_SUMMARY, 1 << 8, 1 << 23, 1 << 30, 1 << 31):
        assert ok(flags=bit) == ERR_FLAGS and ok(flags=bit | N.FLAG_ENV_DQN | N.FLAG_RESET_SHAPING) == ERR_FLAGS, bit
    assert ok(B=0) == 0 and ok(steps=0) == 0
    assert ok(B=0, boards=None) == ERR_NULL and ok(steps=0, weights=0x3008) == ERR_ALIGN
    assert ok(B=0, flags=N.FLAG_INDEPENDENT) == ERR_FLAGS


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
def test_refused_calls_write_nothing(pkg, dev, fam):
    """Each entry point refused for its LAST check on real buffers (and the lookup once for a missing legal_out): the
    weights, boards, aux, both outputs, both statistics vectors and status keep every byte."""
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
    look, play = getattr(L, f"q2048_{fam}_search_lookup"), getattr(L, f"q2048_{fam}_search_play_rollout")
    calls = [
        look(p(V), p(boards), B, p(q_out) + 8, p(legal_out), None),
        look(p(V), p(boards), B, p(q_out), None, None),
        look(p(V), p(boards), -1, p(q_out), p(legal_out), None),
        play(p(boards), p(aux), p(V), B, 3, nan, 1, 0, 0, 0, p(si), p(sf), p(status), None),
        play(p(boards), p(aux), p(V), B, 3, 0.0, 1, 0, 0, 1 << 8, p(si), p(sf), p(status), None),
        play(p(boards), p(aux), p(V), B, -1, 0.0, 1, 0, 0, 0, p(si), p(sf), p(status), None),
    ]
    P.sync(dev)
    assert calls == [ERR_ALIGN, ERR_NULL, ERR_SIZE, ERR_RANGE, ERR_FLAGS, ERR_SIZE]
    for t, b in zip(everything, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "a refused call wrote"
    assert_base_unwritten(fam, dev, "a refused call wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 2. crafted boards
# ---------------------------------------------------------------------------------------------------------------
def lone_tile(cell):
    b = np.zeros(16, np.uint8)
    b[cell] = 1
    return b


ONE_PAIR = np.array([1, 1, 3, 4, 5, 6, 7, 8, 1, 2, 3, 4, 5, 6, 7, 8], np.uint8)       # full; the only equal neighbours: cells 0, 1
ONE_MOVE = np.array([1, 2, 3, 4] + [0] * 12, np.uint8)                                # a full row against its wall: only "down"
# moving left gives a board with ONE empty cell (15), between a 4 (cell 14) and a 16 (cell 11): a 2 there leaves no
# move, a 4 there merges with cell 14
ZERO_BEST = np.array([3, 4, 3, 4, 4, 3, 4, 3, 3, 4, 3, 4, 4, 3, 0, 2], np.uint8)


def aliased_boards(O):
    """Mid-game boards with cells of 16 and 17 planted: they index as 0 and 1 and are not empty."""
    b = AV.midgame(O)[0][1000:1016].copy()
    for i in range(len(b)):
        filled = np.flatnonzero(b[i])
        b[i, filled[0]] = 16
        b[i, filled[-1]] = 17
    b[0, :2] = 16                                                        # a pair of 16s merges into a 17
    return b


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
def test_crafted_boards(pkg, O, dev, fam):
    L = lib(pkg, dev)
    boards = np.stack([lone_tile(0), lone_tile(5), lone_tile(15), ONE_PAIR, ONE_MOVE, P.DEAD.numpy(), ZERO_BEST])
    want, legal, best = assert_rows(L, O, fam, dev, boards, "crafted boards")
    counts = [len(model_nodes(*[x[i:i + 1] for x in model_moves(O, boards)[::2]])) for i in range(len(boards))]
    assert mask_of(legal).tolist() == [0b1100, 0b1111, 0b0011, 0b0101, 0b1000, 0, mask_of(legal)[6]]
    assert counts[:6] == [60, 120, 60, 4, 24, 0], "lone tiles: 15 empty cells per legal move; cell 5 fills all 120 slots"
    assert not bits(want[5]).any(), "no legal move: the row is all +0.0"
    assert (bits(want[:5]) != 0).sum() == 2 + 4 + 2 + 2 + 1, "an illegal move reads +0.0, a legal one its mean"
    # ZERO_BEST: the model sees the afterstate with one empty cell, a dead board behind the 2 and a live one behind the 4
    moved, score, zlegal = model_moves(O, ZERO_BEST[None])
    assert zlegal[0, 0] and int((moved[0, 0] == 0).sum()) == 1 and moved[0, 0, 15] == 0 and score[0, 0] == 0
    nodes = model_nodes(moved, zlegal & np.array([True, False, False, False]))
    nq, nlegal, _ = model_eval(O, fam, nodes)
    b2, b4 = model_best(nq, nlegal)
    assert not nlegal[0].any() and bits(np.array([b2]))[0] == 0 and nlegal[1].any() and b4 != 0
    assert bits(want[6, :1])[0] == bits(np.array([F32((9.0 * 0.0 + float(b4)) / 10.0)]))[0], "a 0.0f best enters the sum"
    # cells of 16 and 17
    al = aliased_boards(O)
    assert_rows(L, O, fam, dev, al, "cells of 16 and 17")
    low = al & 15
    assert (bits(model_search(O, fam, low)[0]) != bits(model_search(O, fam, al)[0])).any(), "16 is a tile, not an empty cell"
    assert_base_unwritten(fam, dev, "the lookup wrote the weights")


def midgame_model(O, fam):
    """257 of the oracle's mid-game boards and the model's searched and greedy rows of them, computed once."""
    key = ("mid", fam)
    if key not in _SHARED:
        boards = AV.midgame(O)[0][2000:2257]
        q, legal, _ = model_search(O, fam, boards)
        greedy_q, greedy_legal, _ = model_eval(O, fam, boards)
        assert np.array_equal(legal, greedy_legal)
        for a in (q, legal, greedy_q):
            a.setflags(write=False)
        _SHARED[key] = (boards, q, legal, greedy_q)
    return _SHARED[key]


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
def test_searched_and_greedy_choices_differ(pkg, O, dev, fam):
    """On mid-game boards the searched first maximum is, for some boards, another move than the greedy one (by the
    model), and the library's rows pick the model's moves."""
    boards, q, legal, greedy_q = midgame_model(O, fam)
    searched, greedy = AV.model_greedy(q, legal), AV.model_greedy(greedy_q, legal)
    assert 0 < int((searched != greedy).sum()) < len(boards)
    got, mask = search_lookup(lib(pkg, dev), fam, dev, boards)
    assert np.array_equal(AV.model_greedy(got.view(F32), legal), searched) and np.array_equal(mask, mask_of(legal))


# ---------------------------------------------------------------------------------------------------------------
# 3. batch edges, and the device against the twin
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
def test_batch_edges(pkg, O, dev, fam, B):
    """The last B of the 257 mid-game boards (so that every B starts on another board): full rows and masks."""
    boards, q, legal, _ = midgame_model(O, fam)
    got, mask = search_lookup(lib(pkg, dev), fam, dev, boards[-B:])
    assert_same_bits(got.view(F32), q[-B:], f"B = {B}")
    assert np.array_equal(mask, mask_of(legal[-B:]))
    assert_base_unwritten(fam, dev, "the lookup wrote the weights")


@pytest.mark.gpu
@pytest.mark.parametrize("fam", FAMILIES)
def test_device_equals_twin(pkg, fam):
    """4,096 random boards (cells 0..15, a third of them emptied), full rows and masks: the device's bits are the twin's."""
    rng = np.random.default_rng(4096)
    boards = K.random_boards(rng, 4096)
    boards[rng.random(boards.shape) < 0.33] = 0
    N = pkg._native
    host, hmask = search_lookup(N.host_lib(), fam, "cpu", boards)
    got, mask = search_lookup(N.lib(), fam, "cuda:0", boards)
    assert_same_bits(got.view(F32), host.view(F32), "device and twin")
    assert np.array_equal(mask, hmask) and len(set(mask.tolist())) > 4


# ---------------------------------------------------------------------------------------------------------------
# 4. the player
# ---------------------------------------------------------------------------------------------------------------
STEPS, CUTS = 40, (1, 7, 32)
PLAYER_CASES = [(fam, B, eps, profile, rss) for fam in FAMILIES for B in (5, 65) for eps in (0.0, 0.3)
                for profile, rss in (("shaped", False), ("shaped", True), ("nopenalty", False), ("nopenalty", True))
                if fam == "av" or not rss]


def assert_order_free_sum(got, terms, what):
    """A float64 statistic is the sum of `terms` accumulated in an order nobody fixes (atomics on the device, one
    partial sum per host thread on the twin).  If every term is a multiple of a quantum q and sum |t| < 2^53 q, every
    partial sum of every order is exactly representable and the statistic is THE sum: compared exactly.  Otherwise each
    of the len(terms) - 1 additions rounds by at most half an ulp of a partial sum that is at most sum |t| in
    magnitude, in the model's order and in the library's: that, twice, is the bound -- the precision of the format
    for this many additions, not a tolerance on the values."""
    terms = [float(t) for t in terms]
    total, mag = sum(terms), sum(abs(t) for t in terms)
    if not terms:
        assert got == 0.0, what
        return
    quantum = min([_lowest_bit(t) for t in terms if t != 0.0], default=1.0)
    if mag / quantum < 2.0 ** 53:
        assert got == total, f"{what}: {got!r} != {total!r} (every order gives the same double)"
    else:
        bound = 2.0 * (len(terms) - 1) * 2.0 ** -53 * mag
        assert abs(got - total) <= bound, f"{what}: {got!r} vs {total!r}, bound {bound!r}"


def _lowest_bit(t):
    """The value of the lowest set bit of the double t != 0."""
    m, e = np.frexp(abs(float(t)))
    m = int(m * 2 ** 53)
    return float(m & -m) * 2.0 ** (int(e) - 53)


def crowded_start(pkg, B, profile, rss):
    """The crowded start of the other player tests (test_row_tuple_player.midgame), built on the CPU twin so that both
    devices and the model start from the same bytes."""
    env, dead = AV.midgame_env(pkg, "cpu", B, profile, rss)
    return env.state_dict(), dead


def env_from(pkg, dev, B, profile, rss, sd):
    env = P.make_env(pkg, dev, B, profile, rss)
    env.load_state_dict(sd)
    return env


def model_play(pkg, O, fam, B, eps, profile, rss):
    """The model loop, once per case: the searched row, the player's draw contract (test_row_tuple_player.model_actions),
    the env's four-call step and reset on the CPU twin with the same draws.
    -> (start state, boards, aux, ctr, integer statistics, {float statistic: its terms}, boards of the GREEDY player)"""
    key = ("play", fam, B, eps, profile, rss)
    if key in _SHARED:
        return _SHARED[key]
    N = pkg._native
    sd, dead = crowded_start(pkg, B, profile, rss)
    model = env_from(pkg, "cpu", B, profile, rss, sd)
    si = np.zeros(N.NSTAT_I, np.int64)
    terms = {N.SF_RETURN: [], N.SF_RETURN_SQ: [], N.SF_REWARD: []}
    for _ in range(STEPS):
        q, legal, _ = model_search(O, fam, model.boards.numpy())
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
    greedy_env = env_from(pkg, "cpu", B, profile, rss, sd)
    random_agent(pkg, fam, "cpu").play_rollout(greedy_env, STEPS, epsilon=eps)
    _SHARED[key] = (sd, model.boards.clone(), model.aux.clone(), model.ctr, si, terms, greedy_env.boards.clone())
    return _SHARED[key]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("fam,B,eps,profile,rss", PLAYER_CASES)
def test_player_against_the_model(pkg, O, dev, fam, B, eps, profile, rss):
    """40 steps in launches of 1 + 7 + 32 from crowded boards with dead boards in front: boards, aux bytes, env.ctr, the
    integer statistics vector and the float64 one against the model loop; the weights, the training statistics and
    `status` are not written; episodes end inside the span; and at epsilon 0 the greedy player, started from the same
    bytes, ends on other boards -- the row handed to the choice really is the searched one."""
    N = pkg._native
    sd, boards, aux, ctr, si, terms, greedy_boards = model_play(pkg, O, fam, B, eps, profile, rss)
    env = env_from(pkg, dev, B, profile, rss, sd)
    agent = random_agent(pkg, fam, dev)
    agent.status.fill_(0x777)
    train_stats = agent.stats_i.clone(), agent.stats_f.clone()
    for c in CUTS:
        agent.search_rollout(env, c, epsilon=eps)
    P.sync(dev)
    assert torch.equal(env.boards.cpu(), boards), "boards differ"
    assert torch.equal(env.aux.cpu(), aux), "aux records differ"
    assert env.ctr == ctr == P.WARM + STEPS
    got_i, got_f = (t.cpu().numpy() for t in agent._play_stats)
    assert np.array_equal(got_i, si), f"integer statistics: {got_i.tolist()} != {si.tolist()}"
    assert si[N.ST_STEPS] == B * STEPS and si[N.ST_EPISODES] > 0
    for k in range(N.NSTAT_F):
        assert_order_free_sum(float(got_f[k]), terms.get(k, []), f"float statistic {k}")
    if eps == 0.0:
        assert si[N.ST_EXPLORE] == 0
        assert not torch.equal(boards, greedy_boards), "the searched player played the greedy player's games"
    else:
        assert 0.1 * B * STEPS < si[N.ST_EXPLORE] < 0.5 * B * STEPS
    assert_base_unwritten(fam, dev, "the player wrote to the weights")
    assert torch.equal(agent.stats_i, train_stats[0]) and torch.equal(agent.stats_f, train_stats[1])
    assert int(agent.status.item()) == 0x777, "status: required, never written"


# ---------------------------------------------------------------------------------------------------------------
# 5. the Python surface
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("dev", DEVICES)
def test_python_surface(pkg, O, dev, fam):
    """`search_lookup` returns (float32 [B, 4], uint8 [B]) on the agent's device, `search_rollout` advances env.ctr and
    fills `play_stats`, and both refuse what `play_rollout` refuses: a 5x5 env, an env on another device; nothing of a
    row-tuple checkpoint is promoted."""
    boards, q, legal, _ = midgame_model(O, fam)
    agent = random_agent(pkg, fam, dev)
    got, mask = agent.search_lookup(t8(dev, boards[:33]))
    assert got.dtype == torch.float32 and tuple(got.shape) == (33, 4) and got.device == agent.device
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (33,) and mask.device == agent.device
    assert_same_bits(got, q[:33], "search_lookup")
    assert np.array_equal(mask.cpu().numpy(), mask_of(legal[:33]))
    env = P.make_env(pkg, dev, 9)
    agent.search_rollout(env, 3)
    agent.search_rollout(env, 2, epsilon=1.0)
    P.sync(dev)
    st = agent.play_stats()
    assert env.ctr == 5 and st["steps"] == 45 and st["explored"] == 18 and st["valid_moves"] == 45
    assert agent.stats()["steps"] == 0, "the training statistics never see the player"
    with pytest.raises(ValueError):
        agent.search_rollout(pkg.BatchedGame2048Env(8, 5, dev, agent.seed, agent.env_id0), 1)
    with pytest.raises(ValueError):
        agent.search_lookup(torch.zeros((4, 25), dtype=torch.uint8, device=dev))
    elsewhere = types.SimpleNamespace(device=torch.device("meta"), board_size=4, num_envs=8)     # refused before it is read
    with pytest.raises(ValueError, match="different devices"):
        agent.search_rollout(elsewhere, 1)
    if dev != "cpu":
        with pytest.raises(ValueError, match="different devices"):
            agent.search_rollout(P.make_env(pkg, "cpu", 8), 1)
    with pytest.raises(ValueError):
        agent.load_row_tuple(P.make_agent(pkg, "cpu").state_dict())
    assert env.ctr == 5 and agent.play_stats()["steps"] == 45
    assert_base_unwritten(fam, dev, "the surface wrote to the weights")
