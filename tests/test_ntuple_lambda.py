"""TD(lambda) with a truncated trace for the 6-tuple afterstate network (q2048_nt_choose_ex, q2048_nt_lambda_update,
q2048_nt_lambda_fused_rollout): V = float32 [4, 2^24] beside a caller-owned trace uint64 [B, 4] = {n, key_1, key_2,
key_3}, against a numpy model that applies the six steps of include/q2048.h literally, lane after lane, and
BatchedNTupleAgent(trace_lambda=...) with its checkpoint.  (The scripts: test_ntuple_lambda_scripts.py.)

Which test executes which kernel (device) / function (CPU twin):
  k_nt_choose_ex             test_choose_ex, the loop of test_fused_one_lane_many_steps
  k_nt_lambda_update         test_update_where_lanes_cannot_race, test_shared_weights_inside_a_lane,
                             test_illegal_move_and_bad_action, test_racing_update_at_65536_lanes_properties, the loop of
                             test_fused_one_lane_many_steps
  k_nt_lambda_fused_rollout  test_fused_one_lane_many_steps, test_fused_one_learning_step,
                             test_racing_fused_at_65536_lanes_properties, the checkpoint tests
  k_nt_update / k_nt_fused_rollout through the new entry points   test_depth_zero_is_the_plain_learner
  the argument checks        test_abi, test_argument_errors_need_no_device, test_refused_calls_write_nothing

Every comparison is exact: float32 bit patterns over all 256 MiB of V, and the trace byte for byte.  There is no
tolerance: d_k is one float64 expression rounded once (lr * 0.03125 is exact, L_k a float64 product in the stated
association), and a written entry is one float32 addition.  A trace handed in with n > h (the tests do that) has all its
n keys updated once and is truncated by the push: the six steps, literally."""
import os

import numpy as np
import pytest
import torch

import test_afterstate as AV
import test_line_tuple as LT
import test_ntuple as NT
import test_row_tuple_player as P

REPO, DEVICES, F32, NIDX, BAD_ACTION = NT.REPO, NT.DEVICES, NT.F32, NT.NIDX, NT.BAD_ACTION
ERR_NULL, ERR_SIZE, ERR_ALIGN, ERR_RANGE = NT.ERR_NULL, NT.ERR_SIZE, NT.ERR_ALIGN, NT.ERR_RANGE
lib, t8, t32, bits, assert_same_bits = NT.lib, NT.t8, NT.t32, NT.bits, NT.assert_same_bits
base_values, base_on = NT.base_values, NT.base_on
NAMES = ("q2048_nt_choose_ex", "q2048_nt_lambda_update", "q2048_nt_lambda_fused_rollout")
MAX_CANDIDATES = 6000
U64 = np.uint64
PP = np.arange(4)[:, None]
_SHARED = {}


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def key_of(board):
    """cell 4r + c (its low nibble) in nibble 4r + c -> a Python int below 2^64"""
    return sum((int(c) & 15) << (4 * i) for i, c in enumerate(np.asarray(board).reshape(16)))


def board_of(key):
    return np.array([(int(key) >> (4 * i)) & 15 for i in range(16)], np.uint8)


def trace_rows(rows):
    """[(n, k1, k2, k3), ...] -> uint64 [B, 4]"""
    return np.array([[U64(w) for w in r] for r in rows], U64).reshape(-1, 4)


def tt(dev, trace):
    """uint64 [B, 4] -> an int64 tensor on `dev` (the same bytes)"""
    return torch.from_numpy(np.ascontiguousarray(trace).view(np.int64).copy()).to(dev)


def trace_of(t):
    return t.cpu().numpy().view(U64)


def model_lambda_update(O, V, trace, s, actions, s2, done, cut, lr, gamma, lam, h, inplace=False):
    """The six steps, lane after lane on one array.
    -> (values, trace uint64 [B, 4], status word, per lane the list of the boards whose 32 entries were addressed)"""
    V, status = (V if inplace else V.copy()), 0
    trace = None if trace is None else trace.copy()
    addressed = [[] for _ in range(len(s))]
    for i in range(len(s)):
        a = int(actions[i])
        if a > 3:
            status |= BAD_ACTION
            continue
        x, _, legal = O.move(s[i], a)
        if not legal:
            if done[i] and h > 0:
                trace[i] = 0                      # no weight moves, nothing is pushed; the episode's trace ends
            continue
        n, keys = 0, [0, 0, 0]
        if h > 0:
            n, keys = min(int(trace[i, 0]), 3), [int(k) for k in trace[i, 1:]]
            if cut is not None and cut[i]:        # 1.
                n, keys = 0, [0, 0, 0]
        q2, legal2, _ = NT.model_eval(O, V, s2[i:i + 1])
        live = 1.0 if (not done[i]) and legal2.any() else 0.0
        target = (gamma * float(NT.model_best(q2, legal2)[0])) * live
        err = target - float(NT.model_v(V, x[None])[0])                  # 2. float64
        d0 = F32((lr * 0.03125) * err)                                    # 3.
        idx = NT.model_idx(x[None])[0]
        V[PP, idx] = V[PP, idx] + d0
        addressed[i].append(x)
        if h == 0:
            continue
        L = lam
        for k in range(n):                                                # 4. ascending, each after the stores before
            dk = F32(((lr * 0.03125) * L) * err)
            b = board_of(keys[k])
            idx = NT.model_idx(b[None])[0]
            V[PP, idx] = V[PP, idx] + dk
            addressed[i].append(b)
            L = L * lam
        if done[i]:                                                       # 6.
            trace[i] = 0
        else:                                                             # 5.
            new = ([key_of(x), keys[0], keys[1]][:h] + [0, 0, 0])[:3]
            trace[i] = [U64(min(n + 1, h))] + [U64(k) for k in new]
    return V, trace, status, addressed


def ids_of_boards(boards):
    return set(NT.entry_ids(np.stack(boards)).ravel().tolist()) if len(boards) else set()


def lambda_update(L, dev, weights, trace, s, actions, s2, done, cut, lr, gamma, lam, h):
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ts, ts2, ta, td = t8(dev, s), t8(dev, s2), t8(dev, actions), t8(dev, done)
    tc = None if cut is None else t8(dev, cut)
    assert L.q2048_nt_lambda_update(weights.data_ptr(), None if trace is None else trace.data_ptr(), ts.data_ptr(),
                                    ta.data_ptr(), ts2.data_ptr(), td.data_ptr(), None if tc is None else tc.data_ptr(),
                                    len(s), lr, gamma, lam, h, status.data_ptr(), None) == 0
    for t, a in ((ts, s), (ts2, s2), (ta, actions), (td, done)):
        assert np.array_equal(t.cpu().numpy(), a), "an input was written"
    return int(status.item())


def assert_trace_invariants(trace, h, what):
    n = trace[:, 0]
    assert (n <= U64(h)).all(), f"{what}: n > h"
    beyond = np.arange(1, 4)[None, :] > n[:, None].astype(np.int64)
    assert (trace[:, 1:][beyond] == 0).all(), f"{what}: a word beyond n is not zero"


def make_agent(pkg, dev, eps=0.3, lr=0.1, gamma=0.95, seed=P.SEED, id0=P.ID0, epochs=100, lam=0.5, depth=3):
    kw = {} if lam is None else {"trace_lambda": lam, "trace_depth": depth}
    return pkg.BatchedNTupleAgent(epochs, learning_rate=lr, discount_factor=gamma, exploration_rate=eps, seed=seed,
                                  env_id0=id0, device=dev, **kw)


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
    C = N.C
    res, args = N._SIGNATURES["q2048_nt_choose"]
    assert N._SIGNATURES["q2048_nt_choose_ex"] == (res, args[:-1] + [C.c_void_p, args[-1]])
    res, args = N._SIGNATURES["q2048_nt_update"]          # trace after weights, cut after done, lambda and h after gamma
    assert N._SIGNATURES["q2048_nt_lambda_update"] == \
        (res, args[:1] + [C.c_void_p] + args[1:5] + [C.c_void_p] + args[5:8] + [C.c_double, C.c_int] + args[8:])
    res, args = N._SIGNATURES["q2048_nt_fused_rollout"]
    assert N._SIGNATURES["q2048_nt_lambda_fused_rollout"] == \
        (res, args[:3] + [C.c_void_p] + args[3:8] + [C.c_double, C.c_int] + args[8:])
    assert N.host_lib().q2048_abi_version() == N.lib().q2048_abi_version() == N.ABI_VERSION


def entry_points(L):
    a = [(k + 1) << 32 for k in range(9)]
    nan, inf = float("nan"), float("inf")
    # name: (function, good arguments, required pointers, 16-byte aligned pointers, position of B, {scalar: refused},
    #        positions of weights, trace and h)
    return {
        "nt_lambda_update": (L.q2048_nt_lambda_update,
                             [a[0], a[6], a[1], a[2], a[3], a[4], a[7], 64, 0.1, 0.97, 0.5, 3, a[5], None],
                             (0, 1, 2, 3, 4, 5, 12), (0, 1, 2, 4), 7,
                             {8: (nan,), 9: (nan,), 10: (-0.1, 1.5, inf, nan), 11: (-1, 4)}, (0, 1, 11)),
        "nt_lambda_fused_rollout": (L.q2048_nt_lambda_fused_rollout,
                                    [a[0], a[1], a[2], a[6], 64, 2, 0.3, 0.1, 0.97, 0.5, 3, 3, 50, 0, None, None, a[3], None],
                                    (0, 1, 2, 3, 16), (0, 1, 2, 3), 4,
                                    {6: (-0.1, 1.5, nan), 7: (nan,), 8: (nan,), 9: (-0.1, 1.5, inf, nan), 10: (-1, 4)},
                                    (2, 3, 10)),
    }


@pytest.mark.parametrize("which", ["hip", "host"])
def test_argument_errors_need_no_device(pkg, which):
    """The order of the q2048_nt_* counterparts -- B, NULL, alignment, (steps,) the scalars -- with the trace directly
    after the weights in the NULL list (unless h == 0) and in the alignment list, h outside 0..3 and lambda outside
    [0, 1] or not finite refused with Q2048_ERR_RANGE: on both libraries, with made-up addresses, so nothing behind them
    may be touched (B == 0 and steps == 0 are no-ops)."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    nan, big = float("nan"), (2 ** 31 - 1) * 256 + 1
    table = entry_points(L)
    for name, (fn, good, pointers, aligned, b_pos, scalars, (w_pos, t_pos, h_pos)) in table.items():
        def call(**kw):
            args = list(good)
            for pos, value in kw.items():
                args[int(pos[1:])] = value
            return fn(*args)

        bad_scalar = {f"p{pos}": values[-1] for pos, values in scalars.items()}
        bad_align = {f"p{pos}": good[pos] + 8 for pos in aligned}
        assert t_pos in pointers and t_pos in aligned and t_pos == w_pos + 1
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
        for lam in (0.0, 1.0):
            for h in (0, 1, 2, 3):
                assert call(**{f"p{h_pos - 1}": lam, f"p{h_pos}": h, f"p{b_pos}": 0}) == 0, f"{name}: lambda {lam}, h {h}"
        assert call(**{f"p{b_pos}": 0}) == 0, f"{name}: B = 0"
        assert call(**{f"p{b_pos}": 0, f"p{pointers[0]}": None}) == ERR_NULL, f"{name}: B = 0 is checked first"
        assert call(**{f"p{t_pos}": None, f"p{h_pos}": 0, f"p{b_pos}": 0}) == 0, f"{name}: h = 0 needs no trace"
        assert call(**{f"p{t_pos}": None, f"p{h_pos}": 1, f"p{b_pos}": 0}) == ERR_NULL, f"{name}: h = 1 needs one"
    fn, good = table["nt_lambda_update"][:2]
    args = list(good)
    args[6], args[7] = None, 0                                          # cut may be NULL
    assert fn(*args) == 0
    fn, good = table["nt_lambda_fused_rollout"][:2]
    for steps, eps, code in ((-1, nan, ERR_SIZE), ((1 << 30) + 1, nan, ERR_SIZE), (0, 0.3, 0), (0, nan, ERR_RANGE)):
        args = list(good)
        args[5], args[6] = steps, eps                                   # steps before epsilon
        assert fn(*args) == code, f"nt_lambda_fused_rollout: steps = {steps}"
    a = [(k + 1) << 32 for k in range(4)]                               # q2048_nt_choose_ex checks as q2048_nt_choose
    ex = L.q2048_nt_choose_ex
    assert ex(a[0], a[1], 0, 0.3, 1, 0, 0, a[2], None, None) == 0 and ex(a[0], a[1], 0, 0.3, 1, 0, 0, a[2], a[3], None) == 0
    assert ex(a[0], a[1], 0, 0.3, 1, 0, 0, None, a[3], None) == ERR_NULL and ex(None, a[1], 0, 1.5, 1, 0, 0, a[2], a[3], None) == ERR_NULL
    assert ex(a[0] + 8, a[1], 0, 1.5, 1, 0, 0, a[2], a[3], None) == ERR_ALIGN and ex(a[0], a[1], 0, 1.5, 1, 0, 0, a[2], a[3], None) == ERR_RANGE
    assert ex(a[0], a[1], -1, 0.3, 1, 0, 0, None, a[3], None) == ERR_SIZE


@pytest.mark.parametrize("dev", DEVICES)
def test_refused_calls_write_nothing(pkg, dev):
    """Both learner entry points refused on real buffers -- bad h, bad lambda, NaN lambda, a misaligned and a NULL
    trace -- : V, trace, boards, aux, statistics and status keep every byte."""
    L, B = lib(pkg, dev), 64
    nan = float("nan")
    V = base_on(dev)
    rng = np.random.default_rng(1)
    boards = t8(dev, NT.K.random_boards(rng, B))
    trace = torch.full((B + 1, 4), 0x0123456789ABCDE, dtype=torch.int64, device=dev)
    trace[:, 0] = 2
    aux = torch.full((B, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    acts = torch.full((B,), 2, dtype=torch.uint8, device=dev)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    si, sf = torch.full((64,), 7, dtype=torch.int64, device=dev), torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((1,), 0x777, dtype=torch.int32, device=dev)
    everything = (boards, trace, aux, acts, done, si, sf, status)
    before = [t.clone() for t in everything]
    p = lambda t: t.data_ptr()      # noqa: E731
    up = lambda tr, lam, h: L.q2048_nt_lambda_update(p(V), tr, p(boards), p(acts), p(boards), p(done), p(done), B, 0.1,  # noqa: E731
                                                     0.9, lam, h, p(status), None)
    fu = lambda tr, lam, h: L.q2048_nt_lambda_fused_rollout(p(boards), p(aux), p(V), tr, B, 3, 0.3, 0.1, 0.9, lam, h, 1, 0,  # noqa: E731
                                                            0, p(si), p(sf), p(status), None)
    calls = []
    for fn in (up, fu):
        calls += [fn(p(trace), 0.5, 4), fn(p(trace), 0.5, -1), fn(p(trace), 1.5, 3), fn(p(trace), -0.5, 3), fn(p(trace), nan, 3),
                  fn(p(trace), float("inf"), 3), fn(p(trace) + 8, 0.5, 3), fn(None, 0.5, 3)]
    P.sync(dev)
    assert calls == [ERR_RANGE] * 6 + [ERR_ALIGN, ERR_NULL] + [ERR_RANGE] * 6 + [ERR_ALIGN, ERR_NULL]
    for t, b in zip(everything, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "a refused call wrote"
    NT.assert_base_unwritten(dev, "a refused call wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 2. q2048_nt_choose_ex
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_choose_ex(pkg, O, dev, B):
    """Actions are q2048_nt_choose's bytes; the flags are the draw contract's -- the first draw of (seed, env id, ctr) is
    below ceil(eps * 2^32) and a move exists -- as 0 / 1; nothing is written behind B; a NULL `explored` is accepted.
    Dead boards and boards with one move are among the lanes."""
    L, V = lib(pkg, dev), base_on(dev)
    seed, id0, ctr, eps = 11, 300, 5, 0.4
    boards = AV.crowded()[1000:1000 + B].copy()
    boards[::7] = P.DEAD.numpy()
    boards[3::11] = P.one_move_board(2)
    want, room = NT.nt_choose(L, dev, V, boards, eps, seed, id0, ctr)
    assert (room == NT.A_CANARY).all()
    tb = t8(dev, boards)
    acts = torch.full((B + NT.ROOM,), NT.A_CANARY, dtype=torch.uint8, device=dev)
    flags = torch.full((B + NT.ROOM,), NT.A_CANARY, dtype=torch.uint8, device=dev)
    assert L.q2048_nt_choose_ex(V.data_ptr(), tb.data_ptr(), B, eps, seed, id0, ctr, acts.data_ptr(), flags.data_ptr(), None) == 0
    acts, flags = acts.cpu().numpy(), flags.cpu().numpy()
    assert np.array_equal(acts[:B], want) and (acts[B:] == NT.A_CANARY).all() and (flags[B:] == NT.A_CANARY).all()
    thr = int(np.ceil(eps * 4294967296.0))
    has_move = NT.model_moves(O, boards)[2].any(axis=1)
    model = np.array([int(O.draws(seed, id0 + i, ctr)[0]) < thr and bool(has_move[i]) for i in range(B)], np.uint8)
    assert np.array_equal(flags[:B], model)
    if B >= 63:
        assert 0 < model.sum() < B and (~has_move).any()
    again = torch.full((B,), NT.A_CANARY, dtype=torch.uint8, device=dev)
    assert L.q2048_nt_choose_ex(V.data_ptr(), tb.data_ptr(), B, eps, seed, id0, ctr, again.data_ptr(), None, None) == 0
    assert np.array_equal(again.cpu().numpy(), want)
    NT.assert_base_unwritten(dev, "choosing wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 3. h == 0 is the plain learner
# ---------------------------------------------------------------------------------------------------------------
def plain_transitions(O, B):
    if ("plain", B) not in _SHARED:
        rng = np.random.default_rng(300 + B)
        s, actions, s2 = NT.nonracing_transitions(O, rng, B)
        assert len(s) == B
        _SHARED[("plain", B)] = (s, actions, s2, (rng.random(B) < 0.3).astype(np.uint8))
    return _SHARED[("plain", B)]


@pytest.mark.parametrize("dev", DEVICES)
def test_depth_zero_is_the_plain_learner(pkg, O, dev):
    """h = 0 with trace == NULL (and cut flags set, lambda 0.5): q2048_nt_lambda_update leaves the bytes of
    q2048_nt_update, q2048_nt_lambda_fused_rollout those of q2048_nt_fused_rollout -- weights, boards, aux, statistics."""
    L, V, B = lib(pkg, dev), base_values(), 257
    s, actions, s2, done = plain_transitions(O, B)
    lr, gamma = 0.1, 0.97
    plain, status = t32(dev, V), torch.zeros(1, dtype=torch.int32, device=dev)
    ts, ts2, ta, td = t8(dev, s), t8(dev, s2), t8(dev, actions), t8(dev, done)
    assert L.q2048_nt_update(plain.data_ptr(), ts.data_ptr(), ta.data_ptr(), ts2.data_ptr(), td.data_ptr(), B, lr, gamma,
                             status.data_ptr(), None) == 0
    weights = t32(dev, V)
    got = lambda_update(L, dev, weights, None, s, actions, s2, done, np.ones(B, np.uint8), lr, gamma, 0.5, 0)
    assert got == int(status.item()) == BAD_ACTION
    assert_same_bits(weights, plain, "h = 0: the update")
    assert not np.array_equal(bits(weights), bits(V))
    del plain, weights
    seed, id0, eps = 5, 77, 0.3
    env_p, agent_p = NT.fused_run(pkg, dev, V, 1, (1, 40), seed, id0, eps, lr, gamma)
    env = pkg.BatchedGame2048Env(1, seed=seed, env_id0=id0, device=dev)
    agent = make_agent(pkg, dev, eps, lr, gamma, seed, id0, depth=0)
    agent.weights.copy_(t32("cpu", V))
    agent.fused_rollout(env, 1)
    agent.fused_rollout(env, 40)
    P.sync(dev)
    assert agent.trace is None and agent.check_status() == 0
    assert torch.equal(env.boards, env_p.boards) and torch.equal(env.aux, env_p.aux)
    assert torch.equal(agent.stats_i, agent_p.stats_i) and torch.equal(agent.stats_f, agent_p.stats_f)
    assert_same_bits(agent.weights, agent_p.weights, "h = 0: the fused learner")
    assert not np.array_equal(bits(agent.weights), bits(V))


# ---------------------------------------------------------------------------------------------------------------
# 4. q2048_nt_lambda_update where lanes cannot race
# ---------------------------------------------------------------------------------------------------------------
def nonracing_lanes(O, B):
    """B lanes (s, a, s', n trace boards, n = lane % 4 before acceptance reorders nothing) from test_ntuple's candidates,
    each with up to three `crowded` boards as its history, accepted lane by lane: ACROSS lanes the entry sets of x and of
    all trace boards (the write set) are disjoint from every other lane's read and write set -- the read set being the
    candidates of s' and the write set.  Within a lane they may overlap.  Built once per B."""
    if ("lanes", B) in _SHARED:
        return _SHARED[("lanes", B)]
    rng = np.random.default_rng(700 + B)
    pool = AV.crowded()
    order = rng.permutation(len(pool))[:MAX_CANDIDATES]
    hist = rng.permutation(len(pool))
    s, a, s2, tr = [], [], [], []
    for n, c in enumerate(order):
        board = pool[c]
        act = 7 if n % 7 == 3 else int(rng.integers(0, 4))
        if n % 11 == 5:
            board, act = P.one_move_board(n % 4), (n + 1) % 4
        x = O.move(board, act)[0] if act <= 3 else board
        s.append(board); a.append(act)      # noqa: E702
        s2.append(P.DEAD.numpy().copy() if n % 5 == 2 else AV.spawned(rng, x))
        tr.append([pool[hist[(3 * n + k) % len(pool)]] for k in range(n % 4)])
    s, a, s2 = np.stack(s), np.array(a, np.uint8), np.stack(s2)
    keep, seen_r, seen_w = [], set(), set()
    for i, (r, w) in enumerate(NT.entry_sets_many(O, s, a.astype(np.int64), s2)):
        if w:                                # a lane that learns also addresses its history
            w = w | ids_of_boards(tr[i])
            r = r | w
        if (w & seen_r) or (r & seen_w):
            continue
        seen_r |= r
        seen_w |= w
        keep.append(i)
        if len(keep) == B:
            break
    assert len(keep) == B, f"only {len(keep)} lanes that cannot race among {MAX_CANDIDATES} candidates"
    trace = trace_rows([[len(tr[i])] + [key_of(b) for b in tr[i]] + [0] * (3 - len(tr[i])) for i in keep])
    done = (rng.random(B) < 0.3).astype(np.uint8)
    cut = (rng.random(B) < 0.3).astype(np.uint8)
    _SHARED[("lanes", B)] = (s[keep], a[keep], s2[keep], trace, done, cut)
    return _SHARED[("lanes", B)]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("h", [1, 2, 3])
@pytest.mark.parametrize("B", [1, 64, 65, 257])
def test_update_where_lanes_cannot_race(pkg, O, dev, B, h):
    """The sequential model is the specification: V over all 256 MiB and the trace byte for byte, for lambda = 0, 0.5
    and 1, on traces preloaded with n = 0..3 mixed over the lanes (n > h included), cut on some lanes, done on some,
    bad and illegal actions among them."""
    L, V = lib(pkg, dev), base_values()
    s, actions, s2, trace, done, cut = nonracing_lanes(O, B)
    lr, gamma = 0.1, 0.97
    if B >= 64:
        assert set(trace[:, 0].tolist()) == {0, 1, 2, 3} and 0 < cut.sum() < B and 0 < done.sum() < B and (actions > 3).any()
    weights = t32(dev, V)
    results = []
    for lam in (0.0, 0.5, 1.0):
        want_v, want_t, want_status, addressed = model_lambda_update(O, V, trace, s, actions, s2, done, cut, lr, gamma, lam, h)
        weights.copy_(t32("cpu", V))
        tr = tt(dev, trace)
        assert lambda_update(L, dev, weights, tr, s, actions, s2, done, cut, lr, gamma, lam, h) == want_status
        assert_same_bits(weights, want_v, f"V, B = {B}, h = {h}, lambda = {lam}")
        assert np.array_equal(trace_of(tr), want_t), f"trace, B = {B}, h = {h}, lambda = {lam}"
        wrote = np.array([len(b) > 0 for b in addressed])
        assert_trace_invariants(want_t[wrote], h, "the model")
        assert (want_t[wrote & (done == 1)] == 0).all() and (want_t[wrote & (done == 0), 0] >= 1).all()
        assert np.array_equal(want_t[~wrote & (done == 0)], trace[~wrote & (done == 0)]), "a lane that learned nothing pushed"
        results.append(want_v)
    if B >= 64:
        deep = [i for i, b in enumerate(addressed) if len(b) > 1]
        assert deep, "no lane with a history it may use"
        assert not np.array_equal(bits(results[0]), bits(results[1])) and not np.array_equal(bits(results[1]), bits(results[2]))
        nocut, _, _, _ = model_lambda_update(O, V, trace, s, actions, s2, done, None, lr, gamma, 0.5, h)
        assert not np.array_equal(bits(nocut), bits(results[1])), "the cut does not show"


# ---------------------------------------------------------------------------------------------------------------
# 5. shared weights inside a lane; illegal moves and bad actions
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_shared_weights_inside_a_lane(pkg, O, dev):
    """One lane per call, h = 3, lambda = 0.5, no cut: (a) the newest trace board IS x: its weights move by d_0 and then
    by d_1 from the moved value; (b) the history holds the empty board (key 0 inside n: four weights, each read eight
    times, move once per turn) and a board with a mirror symmetry; (c) two equal trace keys: their weights move by d_1
    and then by d_2.  The teeth: a model that gathers every key before any store gives other bits in every case."""
    L, V = lib(pkg, dev), base_values()
    lr, gamma, lam, h = 0.1, 0.97, 0.5, 3
    rng = np.random.default_rng(43)
    pool = AV.crowded()
    s = np.stack([pool[5], pool[6], pool[7]])
    actions = np.array([0, 1, 2], np.uint8)
    x = [O.move(s[i], int(actions[i])) for i in range(3)]
    assert all(bool(r[2]) for r in x)
    s2 = np.stack([AV.spawned(rng, x[i][0]) for i in range(3)])
    sym = np.array([5, 6, 6, 5, 7, 8, 8, 7, 0, 0, 0, 0, 9, 10, 10, 9], np.uint8)
    other = key_of(pool[8])
    trace = trace_rows([(2, key_of(x[0][0]), other, 0), (3, 0, key_of(sym), 0), (3, other, key_of(pool[9]), other)])
    done = np.zeros(3, np.uint8)
    weights = t32(dev, V)
    want_v = V.copy()
    for k in range(3):
        sl = slice(k, k + 1)
        _, want_t, _, addressed = model_lambda_update(O, want_v, trace[sl], s[sl], actions[sl], s2[sl], done[sl], None, lr,
                                                      gamma, lam, h, inplace=True)
        tr = tt(dev, trace[sl])
        assert lambda_update(L, dev, weights, tr, s[sl], actions[sl], s2[sl], done[sl], None, lr, gamma, lam, h) == 0
        assert np.array_equal(trace_of(tr), want_t), f"trace of case {k}"
        assert int(want_t[0, 0]) == 3 and int(want_t[0, 1]) == key_of(x[k][0]) and int(want_t[0, 2]) == int(trace[k, 1])
    assert_same_bits(weights, want_v, "V after the three cases")
    # (a): the 32 entries of x moved twice, by d_0 and then by d_1
    err = gamma * float(NT.model_best(*NT.model_eval(O, V, s2[0:1])[:2])[0]) - float(NT.model_v(V, x[0][0][None])[0])
    idx = NT.model_idx(x[0][0][None])[0]
    d0, d1 = F32((lr * 0.03125) * err), F32(((lr * 0.03125) * lam) * err)
    assert d0 != 0 and np.array_equal(bits(want_v[PP, idx]), bits((V[PP, idx] + d0) + d1))
    assert not np.array_equal(bits(want_v[PP, idx]), bits(V[PP, idx] + d1))
    # (b): index 0 of each pattern moved once by d_1 of the second call, the symmetric board's 16 distinct entries by d_2
    assert len(np.unique(NT.entry_ids(np.zeros((1, 16), np.uint8)))) == 4 and len(np.unique(NT.entry_ids(sym[None]))) == 16
    assert all(bits(want_v[p, 0:1])[0] != bits(V[p, 0:1])[0] for p in range(4))


@pytest.mark.parametrize("dev", DEVICES)
def test_illegal_move_and_bad_action(pkg, O, dev):
    """Four lanes with a full trace: a bad action (status bit, nothing else), an illegal move (nothing at all), an illegal
    move with done (the four words zeroed: the step on which the env reports the end -- and no weight), a legal move."""
    L, V = lib(pkg, dev), base_values()
    pool = AV.crowded()
    one = P.one_move_board(0)
    s = np.stack([pool[20], one, one, pool[21]])
    actions = np.array([9, 2, 2, 0], np.uint8)
    assert not O.move(one, 2)[2] and O.move(pool[21], 0)[2]
    s2 = np.stack([pool[20], one, one, AV.spawned(np.random.default_rng(2), O.move(pool[21], 0)[0])])
    done = np.array([1, 0, 1, 0], np.uint8)
    cut = np.array([1, 1, 1, 0], np.uint8)
    trace = trace_rows([(3, key_of(pool[30 + 3 * i]), key_of(pool[31 + 3 * i]), key_of(pool[32 + 3 * i])) for i in range(4)])
    want_v, want_t, want_status, addressed = model_lambda_update(O, V, trace, s, actions, s2, done, cut, 0.1, 0.97, 0.5, 3)
    assert want_status == BAD_ACTION and [len(b) for b in addressed] == [0, 0, 0, 4]
    assert np.array_equal(want_t[:2], trace[:2]) and (want_t[2] == 0).all() and int(want_t[3, 1]) == key_of(addressed[3][0])
    weights, tr = t32(dev, V), tt(dev, trace)
    assert lambda_update(L, dev, weights, tr, s, actions, s2, done, cut, 0.1, 0.97, 0.5, 3) == BAD_ACTION
    assert_same_bits(weights, want_v, "V")
    assert np.array_equal(trace_of(tr), want_t)
    changed = np.flatnonzero((bits(want_v) != bits(V)).ravel())
    assert set(changed.tolist()) <= ids_of_boards(addressed[3]) and len(changed) > 100


# ---------------------------------------------------------------------------------------------------------------
# 6. the fused learner
# ---------------------------------------------------------------------------------------------------------------
def four_call_run(pkg, O, dev, V, B, steps, seed, id0, eps, lr, gamma, lam, h, boards=None, trace=None, learn=True):
    """choose_action (q2048_nt_choose_ex) -> env.step -> update_q_value (q2048_nt_lambda_update with the flags of the
    choice) -> env.reset(done), `steps` times, with the statistics the fused learner counts.
    -> (env, agent, statistics, transitions (s, a, s', done, explored))"""
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    agent = make_agent(pkg, dev, eps, lr, gamma, seed, id0, lam=lam, depth=h)
    agent.weights.copy_(t32("cpu", V))
    if boards is not None:
        env.boards.copy_(torch.from_numpy(boards))
    if trace is not None:
        agent.trace = tt(dev, trace)
    thr = 0 if eps <= 0.0 else int(np.ceil(eps * 4294967296.0))
    st = {"steps": 0, "episodes": 0, "valid_moves": 0, "explored": 0, "score_sum": 0}
    trans = []
    for t in range(steps):
        s = env.boards.cpu().numpy().copy()
        has_move = env.legal_moves().cpu().numpy() != 0
        actions = agent.choose_action(env.boards)
        explored = agent.last_explored.cpu().numpy().copy()
        want = np.array([int(O.draws(seed, id0 + i, t)[0]) < thr and bool(has_move[i]) for i in range(B)], np.uint8)
        assert np.array_equal(explored, want), "last_explored is not the draw contract's flag"
        tb = env.boards.clone()
        s2, reward, done, _ = env.step(actions)
        s2n, a, d = s2.cpu().numpy().copy(), actions.cpu().numpy(), done.cpu().numpy().copy()
        st["steps"] += B
        st["episodes"] += int(d.sum())
        st["valid_moves"] += int((s != s2n).any(axis=1).sum())
        st["score_sum"] += int(env.score.cpu().numpy()[d].sum())
        st["explored"] += int(explored.sum())
        if learn:
            agent.update_q_value(tb, actions, reward, s2, done)
        trans.append((s, a, s2n, d.astype(np.uint8), explored))
        env.reset(done)
    assert agent.check_status() == 0
    return env, agent, st, trans


@pytest.mark.parametrize("dev", DEVICES)
def test_fused_one_lane_many_steps(pkg, O, dev):
    """B = 1, lr 0.1, gamma 0.97, lambda 0.5, h = 3, epsilon 0.3 (cuts and episode ends occur), 300 steps in launches of
    1, 7, 64, 1, 7, 64 and 156, so the trace crosses launch boundaries: one lane is the sequential learner, so the result
    is the four-call loop -- boards, aux, statistics, the trace and all 256 MiB bit for bit -- and the numpy model
    applied to the loop's transitions."""
    seed, id0, eps, lr, gamma, lam, h, cuts = 5, 77, 0.3, 0.1, 0.97, 0.5, 3, (1, 7, 64, 1, 7, 64, 156)
    V = base_values()
    env_loop, loop, st_loop, trans = four_call_run(pkg, O, dev, V, 1, sum(cuts), seed, id0, eps, lr, gamma, lam, h)
    assert st_loop["episodes"] > 0 and 0 < st_loop["explored"] < sum(cuts)
    env = pkg.BatchedGame2048Env(1, seed=seed, env_id0=id0, device=dev)
    agent = make_agent(pkg, dev, eps, lr, gamma, seed, id0, lam=lam, depth=h)
    agent.weights.copy_(t32("cpu", V))
    crossed = 0
    for k in cuts:
        agent.fused_rollout(env, k)
        crossed += int(agent.trace[0, 0].item() > 0)
    assert crossed >= 3, "no launch boundary with a trace in flight"
    assert agent.check_status() == 0
    LT.assert_same_run(env, agent, env_loop, st_loop, "B = 1")
    assert_same_bits(agent.weights, loop.weights, "V after 300 sequential steps")
    assert torch.equal(agent.trace.cpu(), loop.trace.cpu()), "the trace after 300 sequential steps"
    want_v, want_t = V.copy(), np.zeros((1, 4), U64)
    depth = []
    for s, a, s2, d, explored in trans:
        _, want_t, status, addressed = model_lambda_update(O, want_v, want_t, s, a, s2, d, explored, lr, gamma, lam, h,
                                                           inplace=True)
        assert status == 0
        depth.append(len(addressed[0]))
    assert max(depth) == 4 and depth.count(1) > 10 and depth.count(0) > 0, "the run does not use the trace at every depth"
    assert_same_bits(agent.weights, want_v, "the model after 300 sequential steps")
    assert np.array_equal(trace_of(agent.trace), want_t)
    plain = NT.fused_run(pkg, dev, V, 1, (sum(cuts),), seed, id0, eps, lr, gamma)[1]
    assert not np.array_equal(bits(plain.weights), bits(want_v)), "the trace does not show"


def nonracing_fused(pkg, O, V, B, seed, id0, eps):
    """test_ntuple's boards for one fused step whose lanes cannot race, and for every lane n = lane % 4 trace boards from
    the `crowded` pool whose entries meet no entry any lane reads or writes (x, the candidates of s and of s', other
    histories).  -> (boards, trace uint64 [B, 4])"""
    if ("fused", B) in _SHARED:
        return _SHARED[("fused", B)]
    boards = NT.nonracing_boards(pkg, O, V, B, seed, id0, eps)
    _, _, trans = NT.four_call_run(pkg, O, "cpu", V, B, 1, seed, id0, eps, 0.0, 0.0, boards=boards, keep=True)
    s, a, s2, _, _ = trans[0]
    taken = set()
    for r, w in NT.entry_sets_many(O, s, a.astype(np.int64), s2, fused=True):
        taken |= r | w
    pool, nxt, rows = AV.crowded(), 10000, []
    for i in range(B):
        keys = []
        while len(keys) < i % 4:
            ids = ids_of_boards([pool[nxt]])
            if not (ids & taken):
                taken |= ids
                keys.append(key_of(pool[nxt]))
            nxt += 1
            assert nxt < len(pool)
        rows.append([len(keys)] + keys + [0] * (3 - len(keys)))
    _SHARED[("fused", B)] = (boards, trace_rows(rows))
    return _SHARED[("fused", B)]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [65, 257])
def test_fused_one_learning_step(pkg, O, dev, B):
    """One learning step (lr 0.1, gamma 0.97, lambda 0.5, h = 2, epsilon 0.3) on boards whose lanes cannot race, with
    preloaded traces (n = 0..3): the model on the transitions of the four-call loop is the specification.  All 256 MiB
    and the trace bit for bit; boards, aux and statistics equal."""
    seed, id0, eps, lr, gamma, lam, h = 23, 4000, 0.3, 0.1, 0.97, 0.5, 2
    V = base_values()
    boards, trace = nonracing_fused(pkg, O, V, B, seed, id0, eps)
    env_loop, _, st_loop, trans = four_call_run(pkg, O, dev, V, B, 1, seed, id0, eps, lr, gamma, lam, h, boards=boards,
                                                trace=trace, learn=False)
    s, a, s2, d, explored = trans[0]
    want_v, want_t, status, addressed = model_lambda_update(O, V, trace, s, a, s2, d, explored, lr, gamma, lam, h)
    assert status == 0 and 0 < st_loop["explored"] < B and max(len(b) for b in addressed) == 4
    assert sum(len(b) > 1 for b in addressed) > B // 4
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    agent = make_agent(pkg, dev, eps, lr, gamma, seed, id0, lam=lam, depth=h)
    agent.weights.copy_(t32("cpu", V))
    env.boards.copy_(torch.from_numpy(boards))
    agent.trace = tt(dev, trace)
    agent.fused_rollout(env, 1)
    assert agent.check_status() == 0
    LT.assert_same_run(env, agent, env_loop, st_loop, f"B = {B}")
    assert_same_bits(agent.weights, want_v, f"V, B = {B}")
    assert np.array_equal(trace_of(agent.trace), want_t), f"trace, B = {B}"
    assert_trace_invariants(want_t[[len(b) > 0 for b in addressed]], h, "the model")


# ---------------------------------------------------------------------------------------------------------------
# 7. 65,536 racing lanes, by properties only
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_racing_update_at_65536_lanes_properties(pkg, O, dev):
    """65,536 lanes of q2048_nt_lambda_update from zeros, h = 3, lambda = 0.5, no cuts, traces preloaded with n = lane % 4
    keys of mid-game boards: every weight stays finite, the weights written are a subset of the entries the model says
    were addressed (x and the n trace boards of every lane with a legal move), n <= h, words beyond n are zero, and n == 0
    in every lane whose step ended an episode."""
    L, B, h = lib(pkg, dev), 65536, 3
    boards, (moved, _, legal) = AV.midgame(O)
    rng = np.random.default_rng(77)
    actions = rng.integers(0, 4, B).astype(np.uint8)
    took = legal[np.arange(B), actions]
    x = moved[np.arange(B), actions]
    s2 = x.copy()
    done = (rng.random(B) < 0.2).astype(np.uint8)
    hist = [boards[rng.permutation(B)] for _ in range(3)]
    trace = np.zeros((B, 4), U64)
    trace[:, 0] = np.arange(B) % 4
    addressed = np.zeros(4 * NIDX, bool)
    addressed[NT.entry_ids(x[took]).ravel()] = True
    for k in range(3):
        kk = ((hist[k] & 15).astype(U64) << (np.arange(16, dtype=U64) * U64(4))[None, :]).sum(axis=1, dtype=U64)
        use = trace[:, 0] > k
        trace[use, k + 1] = kk[use]
        addressed[NT.entry_ids(hist[k][use & took]).ravel()] = True
    assert int(trace[5, 1]) == key_of(hist[0][5])
    weights, tr = torch.zeros((4, NIDX), dtype=torch.float32, device=dev), tt(dev, trace)
    assert lambda_update(L, dev, weights, tr, boards, actions, s2, done, None, 0.05, 0.9, 0.5, h) == 0
    v = weights.cpu().numpy().ravel()
    changed = np.flatnonzero(v)
    assert np.isfinite(v).all() and np.abs(v[changed]).max() < 1e4
    assert len(changed) and addressed[changed].all(), "a weight no lane addressed was written"
    assert len(changed) > int(addressed.sum()) // 2
    got = trace_of(tr)
    assert_trace_invariants(got, h, "65,536 racing lanes")
    assert (got[done == 1] == 0).all() and (got[took & (done == 0), 0] == np.minimum(trace[took & (done == 0), 0] + U64(1), U64(h))).all()
    assert np.array_equal(got[~took & (done == 0)], trace[~took & (done == 0)])


@pytest.mark.parametrize("dev", DEVICES)
def test_racing_fused_at_65536_lanes_properties(pkg, O, dev):
    """65,536 lanes of the fused learner.  On frozen weights (lr = 0, the base values, epsilon 0.3, 12 steps in launches of
    1 + 10 + 1, from `crowded` boards a few moves from the end of their games, so episodes end on every step) boards, aux and counters are the plain learner's, V keeps its bits, n <= h = 2, words beyond n are zero and
    n == 0 in every lane whose last step ended an episode.  Learning from zeros at epsilon = 1 (an exploring choice reads
    no value, so the run is the four-call loop's whatever the racing writes do): every weight finite and only entries some
    lane's afterstate visited are written (every step is cut: no history is addressed)."""
    B, seed, eps, gamma, h = 65536, 31, 0.3, 0.9, 2
    V = base_values()
    env_p = pkg.BatchedGame2048Env(B, seed=seed, device=dev)
    plain = make_agent(pkg, dev, eps, 0.0, gamma, seed, 0, lam=None)
    plain.weights.copy_(t32("cpu", V))
    env = pkg.BatchedGame2048Env(B, seed=seed, device=dev)
    agent = make_agent(pkg, dev, eps, 0.0, gamma, seed, 0, lam=0.5, depth=h)
    agent.weights = plain.weights                             # frozen: both only read them
    late = torch.from_numpy(np.resize(AV.crowded(), (B, 16)))
    env_p.boards.copy_(late)
    env.boards.copy_(late)
    for k in (1, 10):
        plain.fused_rollout(env_p, k)
        agent.fused_rollout(env, k)
    episodes_before = env.aux.cpu().numpy().view(np.uint32)[:, 3].copy()
    plain.fused_rollout(env_p, 1)
    agent.fused_rollout(env, 1)
    P.sync(dev)
    assert torch.equal(env.boards, env_p.boards) and torch.equal(env.aux, env_p.aux)
    assert torch.equal(agent.stats_i, plain.stats_i)
    # the float sums are atomic additions of the same 786,432 float64 terms in an order that differs from launch to
    # launch: two orders differ by at most n * 2^-53 of the sum of magnitudes, below 1e-10 of it (returns and rewards
    # of these boards are positive but for rare penalties, so each sum is of the order of its sum of magnitudes)
    assert torch.allclose(agent.stats_f, plain.stats_f, rtol=1e-9, atol=0.0)
    st = agent.stats()
    assert st["steps"] == B * 12 and 0 < st["explored"] < st["steps"] and agent.check_status() == 0
    assert_same_bits(agent.weights, V, "lr = 0 wrote V")
    got = trace_of(agent.trace)
    assert_trace_invariants(got, h, "the fused learner")
    ended = env.aux.cpu().numpy().view(np.uint32)[:, 3] != episodes_before
    assert ended.sum() > 100 and (got[ended] == 0).all() and (got[~ended, 0] >= 1).sum() > B // 2
    assert (got[:, 0] == h).sum() > B // 4
    del plain, agent

    steps = 4
    env = pkg.BatchedGame2048Env(B, seed=seed, device=dev)
    agent = make_agent(pkg, dev, 1.0, 0.05, gamma, seed, 0, lam=0.5, depth=3)
    agent.fused_rollout(env, 1)
    agent.fused_rollout(env, steps - 1)
    loop_env = pkg.BatchedGame2048Env(B, seed=seed, device=dev)
    loop = make_agent(pkg, dev, 1.0, 0.05, gamma, seed, 0, lam=None)
    loop.weights = agent.weights                              # an exploring choice reads none
    visited = np.zeros(4 * NIDX, bool)
    for _ in range(steps):
        s = loop_env.boards.cpu().numpy().copy()
        a = loop.choose_action(loop_env.boards)
        _, _, done, _ = loop_env.step(a)
        a = a.cpu().numpy()
        moved, _, legal = NT.model_moves(O, s)
        took = legal[np.arange(B), a]
        visited[NT.entry_ids(moved[np.arange(B), a][took]).ravel()] = True
        loop_env.reset(done)
    P.sync(dev)
    assert torch.equal(env.boards, loop_env.boards) and torch.equal(env.aux, loop_env.aux)
    v = agent.weights.cpu().numpy().ravel()
    changed = np.flatnonzero(v)
    assert np.isfinite(v).all() and np.abs(v[changed]).max() < 1e4
    assert len(changed) and visited[changed].all(), "an entry no lane visited was written"
    assert len(changed) > int(visited.sum()) // 2 and agent.check_status() == 0
    assert_trace_invariants(trace_of(agent.trace), 3, "epsilon = 1")


# ---------------------------------------------------------------------------------------------------------------
# 8. the Python surface and the checkpoint
# ---------------------------------------------------------------------------------------------------------------
def test_constructor_refusals(pkg):
    mk = lambda **kw: pkg.BatchedNTupleAgent(10, device="cpu", **kw)      # noqa: E731
    for kw in ({"trace_lambda": 0.5, "coherence": True}, {"trace_lambda": 0.5, "stage_tiles": (2048,)},
               {"trace_lambda": 1.5}, {"trace_lambda": -0.1}, {"trace_lambda": float("nan")}, {"trace_lambda": "0.5"},
               {"trace_lambda": True}, {"trace_lambda": 0.5, "trace_depth": 4}, {"trace_lambda": 0.5, "trace_depth": -1},
               {"trace_lambda": 0.5, "trace_depth": 1.0}, {"trace_lambda": 0.5, "trace_depth": True}):
        with pytest.raises(ValueError):
            mk(**kw)
    plain = mk()
    assert plain.trace_lambda is None and plain.trace is None and "trace" not in plain.state_dict()
    agent = mk(trace_lambda=0.5)
    assert agent.trace_lambda == 0.5 and agent.trace_depth == 3 and agent.trace is None and agent.last_explored is None
    assert mk(trace_lambda=0, trace_depth=0).trace_depth == 0
    with pytest.raises(ValueError):
        plain.update_q_value(np.zeros((2, 16), np.uint8), [0, 0], [0.0, 0.0], np.zeros((2, 16), np.uint8), [0, 0], cut=[0, 0])


@pytest.mark.parametrize("dev", DEVICES)
def test_last_explored_and_cut(pkg, O, dev):
    """`choose_action` keeps the flags; `update_q_value` uses them once (a second update without a choice raises, so does
    one of another batch size), `cut=` overrides them, and another B than the trace's is refused."""
    V = base_values()
    s, actions, s2, trace, done, cut = nonracing_lanes(O, 65)
    agent = make_agent(pkg, dev, lr=0.1, gamma=0.97, lam=0.5, depth=3)
    agent.weights.copy_(t32("cpu", V))
    with pytest.raises(ValueError, match="choose_action"):
        agent.update_q_value(t8(dev, s), actions, np.zeros(65, F32), t8(dev, s2), done)
    assert agent.trace is None
    agent.trace = tt(dev, trace)
    agent.update_q_value(t8(dev, s), actions, np.zeros(65, F32), t8(dev, s2), done, cut=cut)
    want_v, want_t, status, _ = model_lambda_update(O, V, trace, s, actions, s2, done, cut, 0.1, 0.97, 0.5, 3)
    assert_same_bits(agent.weights, want_v, "update_q_value(cut=...)")
    assert np.array_equal(trace_of(agent.trace), want_t) and status == BAD_ACTION
    with pytest.raises(ValueError):
        agent.check_status()
    agent.status.zero_()
    agent.choose_action(t8(dev, s))
    flags = agent.last_explored.cpu().numpy().copy()
    assert flags.shape == (65,) and set(flags.tolist()) <= {0, 1}
    with pytest.raises(ValueError, match="choose_action"):
        agent.update_q_value(t8(dev, s[:64]), actions[:64], np.zeros(64, F32), t8(dev, s2[:64]), done[:64])
    before = (bits(agent.weights).copy(), trace_of(agent.trace).copy())
    agent.update_q_value(t8(dev, s), actions, np.zeros(65, F32), t8(dev, s2), done)
    want_v2, want_t2, _, _ = model_lambda_update(O, want_v, want_t, s, actions, s2, done, flags, 0.1, 0.97, 0.5, 3)
    assert_same_bits(agent.weights, want_v2, "update_q_value with the flags of choose_action")
    assert np.array_equal(trace_of(agent.trace), want_t2) and not np.array_equal(before[0], bits(agent.weights))
    with pytest.raises(ValueError, match="choose_action"):
        agent.update_q_value(t8(dev, s), actions, np.zeros(65, F32), t8(dev, s2), done)
    with pytest.raises(ValueError, match="lanes"):
        agent.update_q_value(t8(dev, s[:8]), actions[:8], np.zeros(8, F32), t8(dev, s2[:8]), done[:8], cut=cut[:8])
    small = pkg.BatchedGame2048Env(8, 4, dev, agent.seed, agent.env_id0)
    small.ctr = agent.ctr
    with pytest.raises(ValueError, match="lanes"):
        agent.fused_rollout(small, 1)


def lam_state(agent, env):
    return P.learner_state(agent, env) + (agent.trace.cpu(),)


@pytest.mark.parametrize("dev", DEVICES)
def test_checkpoint_resumes_the_run(pkg, dev):
    """120 steps, a checkpoint, a fresh agent and env, 80 more == 200 uninterrupted steps at B = 1 in all of V, the trace,
    boards, aux, statistics, counters and epsilon; the file keeps the family's kind and adds "trace"."""
    def run(cuts):
        env = P.make_env(pkg, dev, 1)
        agent = make_agent(pkg, dev, eps=0.2, epochs=10)
        for k, steps in enumerate(cuts):
            agent.fused_rollout(env, steps)
            agent.decay_exploration(k)
            yield env, agent

    for env, agent in run([120, 80]):
        pass
    whole = lam_state(agent, env)
    del agent
    (env1, agent1), = run([120])
    sd, esd = agent1.state_dict(), env1.state_dict()
    assert sd["kind"] == "ntuple6_afterstate" and set(sd["trace"]) == {"lambda", "depth", "keys"}
    assert sd["trace"]["lambda"] == 0.5 and sd["trace"]["depth"] == 3
    keys = sd["trace"]["keys"]
    assert keys.device.type == "cpu" and keys.dtype == torch.int64 and tuple(keys.shape) == (1, 4) and int(keys[0, 0]) > 0
    env2 = P.make_env(pkg, dev, 1, seed=1, id0=2)
    agent2 = make_agent(pkg, dev, eps=0.1, seed=1, id0=2, epochs=10)
    agent2.load_state_dict(sd)
    env2.load_state_dict(esd)
    P.assert_same_state(lam_state(agent2, env2), lam_state(agent1, env1))      # the round trip
    del agent1, sd
    agent2.fused_rollout(env2, 80)
    agent2.decay_exploration(1)
    P.sync(dev)
    P.assert_same_state(lam_state(agent2, env2), whole)


@pytest.mark.parametrize("dev", DEVICES)
def test_loading_in_every_combination(pkg, dev):
    """plain <- trace file: the traces are ignored and the plain agent plays the games of the trace agent's weights;
    trace <- plain file: same values, empty traces; trace <- trace file of another depth, another B, or with broken keys:
    refused before anything is written."""
    env, tr = P.make_env(pkg, dev, 64), make_agent(pkg, dev)
    tr.fused_rollout(env, 20)
    tr_sd = tr.state_dict()
    assert bool((tr_sd["trace"]["keys"][:, 0] > 0).any())
    plain = make_agent(pkg, dev, lam=None, seed=9, id0=9)
    plain.load_state_dict(tr_sd)
    assert plain.trace is None and "trace" not in plain.state_dict()
    assert torch.equal(P.bits(plain.weights), P.bits(tr.weights)) and plain.ctr == tr.ctr
    games = []
    for player in (plain, tr):
        e = P.make_env(pkg, dev, 96, seed=3, id0=500)
        player.play_rollout(e, 40)
        player.play_rollout(e, 160)
        P.sync(dev)
        stats = player.play_stats()
        player.search_rollout(e, 4)
        P.sync(dev)
        games.append((e.boards.cpu(), e.aux.cpu(), stats))
    assert torch.equal(games[0][0], games[1][0]) and torch.equal(games[0][1], games[1][1]) and games[0][2] == games[1][2]
    assert games[0][2]["steps"] == 96 * 200 and games[0][2]["episodes"] > 0

    plain_sd = dict(plain.state_dict(), ctr=555)
    other = make_agent(pkg, dev, seed=9, id0=9)
    other.trace = torch.full((64, 4), 1, dtype=torch.int64, device=dev)
    other.load_state_dict(plain_sd)
    assert other.ctr == 555 and torch.equal(P.bits(other.weights), P.bits(tr.weights))
    assert not bool(other.trace.any()), "a plain file restarts the traces empty"
    fresh = make_agent(pkg, dev, seed=9, id0=9)
    fresh.load_state_dict(plain_sd)
    assert fresh.trace is None
    fresh.load_state_dict(tr_sd)
    assert torch.equal(fresh.trace.cpu(), tr_sd["trace"]["keys"])
    del other, plain, plain_sd, fresh

    before = lam_state(tr, env)
    keys = tr_sd["trace"]["keys"]
    marked = dict(tr_sd, ctr=999, stats_i=tr_sd["stats_i"] + 1)
    broken_n, broken_word = keys.clone(), keys.clone()
    broken_n[3, 0] = 4
    broken_word[:] = 0
    broken_word[5, 2] = 77
    for wrong in (dict(tr_sd["trace"], depth=2), dict(tr_sd["trace"], keys=keys[:32]), dict(tr_sd["trace"], keys=keys.int()),
                  dict(tr_sd["trace"], keys=keys[:, :3]), dict(tr_sd["trace"], keys=keys.numpy()),
                  dict(tr_sd["trace"], keys=broken_n), dict(tr_sd["trace"], keys=broken_word), "trace"):
        with pytest.raises(ValueError, match="trace"):
            tr.load_state_dict(dict(marked, trace=wrong))
    with pytest.raises(ValueError):
        tr.load_state_dict(dict(marked, weights=marked["weights"][:2]))      # good traces, the rest wrong
    shallow = make_agent(pkg, dev, depth=1)
    with pytest.raises(ValueError, match="depth"):
        shallow.load_state_dict(marked)
    P.sync(dev)
    P.assert_same_state(lam_state(tr, env), before)
    tr.load_state_dict(marked)
    assert tr.ctr == 999 and torch.equal(tr.trace.cpu(), keys)
