"""The staged 6-tuple network (q2048_nts_*): V = float32 [S, 4, 2^24], a table per largest-tile stage, against a numpy
model composed from the models of test_ntuple / test_search / test_search_depth -- `model_eval` with V[stage(board)] per
candidate -- and BatchedNTupleAgent(stage_tiles=...).  (The scripts and the checkpoint: test_ntuple_stages_scripts.py.)

Which test executes which kernel (device) / function (CPU twin):
  k_nts_value, k_nts_lookup, k_nts_choose   test_stages_zero_is_the_plain_network, test_equal_tables_are_invisible,
                                            test_crafted_boards, test_random_boards_reach_every_stage
  k_nts_update                              test_update_where_lanes_cannot_race, the loop of test_one_lane_300_steps
  k_nts_fused_rollout                       test_fused_one_learning_step, test_one_lane_300_steps,
                                            test_racing_learning_at_65536_boards_properties
  k_eval_play_rollout<NtsEvalOf, E>         test_player_equals_the_four_call_loop, test_player_exploration_against_the_model
  k_search_lookup<NtsEvalOf> / k_search2_lookup<NtsEvalOf>   test_search_rows, test_search_batch_edges
  k_search_play_rollout<NtsEvalOf, E> / k_search2_play_rollout<NtsEvalOf, E>   test_searched_player_against_the_model (E = 0;
                                            E = 0..3: test_search_depth.test_searched_player_equals_the_four_call_loop)
  k_nts_promote                             test_promotion, test_promotion_cascade
  the argument checks                       test_abi, test_malformed_specs_and_argument_errors, test_refused_calls_write_nothing

Every comparison is exact, on float32 bit patterns; the learning tests compare all S x 256 MiB.  The stage tables are
per-stage bit transforms of test_ntuple's base values (an XOR of mantissa bits): they differ from each other in EVERY
entry, so an entry read from the wrong table changes bits."""
import os
import subprocess
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import test_afterstate as AV
import test_line_tuple as LT
import test_ntuple as NT
import test_row_tuple_kernels as K
import test_row_tuple_player as P
import test_search as S
import test_search_depth as SD

REPO, DEVICES, F32, NIDX, BAD_ACTION = NT.REPO, NT.DEVICES, NT.F32, NT.NIDX, NT.BAD_ACTION
ERR_NULL, ERR_SIZE, ERR_ALIGN, ERR_RANGE, ERR_FLAGS = NT.ERR_NULL, NT.ERR_SIZE, NT.ERR_ALIGN, NT.ERR_RANGE, NT.ERR_FLAGS
ROOM, Q_CANARY, A_CANARY = K.ROOM, K.Q_CANARY, K.A_CANARY
lib, t8, t32, bits, assert_same_bits = NT.lib, NT.t8, NT.t32, NT.bits, NT.assert_same_bits
model_moves, model_best, mask_of = AV.model_moves, AV.model_best, AV.mask_of
NAMES = ("q2048_nts_value", "q2048_nts_lookup", "q2048_nts_choose", "q2048_nts_update", "q2048_nts_fused_rollout",
         "q2048_nts_play_rollout", "q2048_nts_search_lookup_depth", "q2048_nts_search_play_rollout_depth",
         "q2048_nts_promote")
STAGE_XOR = (0x00000000, 0x00155555, 0x002aaaaa)      # mantissa bits: finite, the same magnitude, another value everywhere
BATCHES = [1, 63, 64, 65, 255, 256, 257]
_SHARED = {}


def spec(*thresholds):
    """the `stages` word of tile exponents t_1 < t_2 < ..."""
    return sum(t << (4 * i) for i, t in enumerate(thresholds))


def tables(S_):
    """float32 [S, 4, 2^24]: table k = the bits of test_ntuple's base values XOR STAGE_XOR[k]; built once, never written"""
    if ("v", S_) not in _SHARED:
        base = bits(NT.base_values())
        v = np.stack([(base ^ np.uint32(STAGE_XOR[k])).view(F32) for k in range(S_)])
        assert np.isfinite(v).all() and all((bits(v[k]) != bits(v[j])).all() for k in range(S_) for j in range(k))
        v.setflags(write=False)
        _SHARED[("v", S_)] = v
    return _SHARED[("v", S_)]


def tables_on(dev, S_):
    """The stage tables on `dev`, uploaded once per device for the tests that only READ them."""
    key = ("t", S_, str(dev))
    if key not in _SHARED:
        _SHARED[key] = t32(dev, tables(S_))
    return _SHARED[key]


def assert_tables_unwritten(dev, S_, what):
    assert np.array_equal(bits(tables_on(dev, S_)), bits(tables(S_))), what


# ---------------------------------------------------------------------------------------------------------------
# the staged model, composed from the plain one
# ---------------------------------------------------------------------------------------------------------------
def model_stage(boards, thr):
    """stage(x) = the number of thresholds t with maxnib(x) >= t, maxnib over the LOW NIBBLES of the cells"""
    m = (np.asarray(boards, np.uint8).reshape(-1, 16) & 15).max(axis=1).astype(np.int64)
    return sum((m >= t).astype(np.int64) for t in thr) if thr else np.zeros(len(m), np.int64)


def model_v(Vs, thr, boards):
    """NT.model_v with V[stage(board)] -> float32 [B]"""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    st, out = model_stage(boards, thr), np.zeros(len(boards), F32)
    for k in np.unique(st):
        out[st == k] = NT.model_v(Vs[k], boards[st == k])
    return out


def model_eval(O, Vs, thr, boards, moves=None):
    """NT.model_eval with every candidate afterstate in the table of its own stage
    -> (q float32 [B, 4], legal bool [B, 4], moved boards, stage of every candidate int [B, 4])"""
    moved, score, legal = moves if moves is not None else model_moves(O, boards)
    q = np.stack([score[:, a].astype(F32) + model_v(Vs, thr, moved[:, a]) for a in range(4)], axis=1)
    assert q.dtype == F32
    return q, legal, moved, np.stack([model_stage(moved[:, a], thr) for a in range(4)], axis=1)


def model_update(O, Vs, thr, s, actions, s2, done, lr, gamma, inplace=False):
    """NT.model_update on table stage(c_act), the target from the STAGED evaluation of s'.
    -> (tables afterwards, status, int [B, 4, 8] written indices or -1, int [B] stage written or -1)"""
    Vs, status = (Vs if inplace else Vs.copy()), 0
    written, wstage = np.full((len(s), 4, 8), -1, np.int64), np.full(len(s), -1, np.int64)
    pp = np.arange(4)[:, None]
    for i in range(len(s)):
        a = int(actions[i])
        if a > 3:
            status |= BAD_ACTION
            continue
        x, _, legal = O.move(s[i], a)
        if not legal:
            continue
        q2, legal2, _, _ = model_eval(O, Vs, thr, s2[i:i + 1])
        live = 1.0 if (not done[i]) and legal2.any() else 0.0
        target = (gamma * float(model_best(q2, legal2)[0])) * live                    # float64
        k = int(model_stage(x[None], thr)[0])
        d = F32((lr * 0.03125) * (target - float(NT.model_v(Vs[k], x[None])[0])))    # rounded once
        idx = NT.model_idx(x[None])[0]
        Vs[k][pp, idx] = Vs[k][pp, idx] + d
        written[i], wstage[i] = idx, k
    return Vs, status, written, wstage


@contextmanager
def staged_search_model(Vs, thr):
    """test_search.model_search / test_search_depth.model_search2 with the staged evaluation at the leaves: their own
    code, `model_eval` handed in (family name "nts": a memo of its own for best_1)."""
    plain = S.model_eval
    S.model_eval = lambda O, fam, boards: model_eval(O, Vs, thr, boards)[:3]
    SD._BEST1["nts"] = {}
    try:
        yield
    finally:
        S.model_eval = plain
        del SD._BEST1["nts"]


# ---------------------------------------------------------------------------------------------------------------
# the entry points, through ctypes alone
# ---------------------------------------------------------------------------------------------------------------
def nts_value(L, dev, W, stages, boards):
    B = len(boards)
    out = torch.full((B + ROOM,), Q_CANARY - (1 << 32), dtype=torch.int32, device=dev)
    tb = t8(dev, boards)
    assert L.q2048_nts_value(W.data_ptr(), stages, tb.data_ptr(), B, out.data_ptr(), None) == 0
    out = out.cpu().numpy().view(np.uint32)
    assert (out[B:] == np.uint32(Q_CANARY)).all(), "values written beyond B"
    return out[:B]


def nts_lookup(L, dev, W, stages, boards):
    B = len(boards)
    out = torch.full((B + ROOM, 4), Q_CANARY - (1 << 32), dtype=torch.int32, device=dev)
    tb = t8(dev, boards)
    assert L.q2048_nts_lookup(W.data_ptr(), stages, tb.data_ptr(), B, out.data_ptr(), None) == 0
    out = out.cpu().numpy().view(np.uint32)
    assert (out[B:] == np.uint32(Q_CANARY)).all(), "rows written beyond B"
    return out[:B]


def nts_choose(L, dev, W, stages, boards, eps, seed=0, env_id0=0, ctr=0):
    B = len(boards)
    out = torch.full((B + ROOM,), A_CANARY, dtype=torch.uint8, device=dev)
    tb = t8(dev, boards)
    assert L.q2048_nts_choose(W.data_ptr(), stages, tb.data_ptr(), B, float(eps), seed, env_id0, ctr, out.data_ptr(),
                              None) == 0
    out = out.cpu().numpy()
    assert (out[B:] == A_CANARY).all(), "actions written beyond B"
    return out[:B]


def nts_search(L, dev, W, stages, boards, depth):
    B = len(boards)
    q = torch.full((B + ROOM, 4), Q_CANARY - (1 << 32), dtype=torch.int32, device=dev)
    legal = torch.full((B + ROOM,), A_CANARY, dtype=torch.uint8, device=dev)
    tb = t8(dev, boards)
    assert L.q2048_nts_search_lookup_depth(W.data_ptr(), stages, tb.data_ptr(), B, depth, q.data_ptr(), legal.data_ptr(),
                                           None) == 0
    P.sync(dev)
    q, legal = q.cpu().numpy().view(np.uint32), legal.cpu().numpy()
    assert (q[B:] == Q_CANARY).all() and (legal[B:] == A_CANARY).all(), "written beyond B"
    return q[:B], legal[:B]


def make_agent(pkg, dev, tiles, eps=0.3, lr=0.1, gamma=0.95, seed=P.SEED, id0=P.ID0, epochs=100, weights=None):
    agent = pkg.BatchedNTupleAgent(epochs, learning_rate=lr, discount_factor=gamma, exploration_rate=eps, seed=seed,
                                   env_id0=id0, device=dev, stage_tiles=tiles)
    if weights is not None:
        agent.weights = weights
    return agent


# ---------------------------------------------------------------------------------------------------------------
# 1. ABI and argument checks
# ---------------------------------------------------------------------------------------------------------------
def test_abi(pkg):
    N = pkg._native
    with open(os.path.join(REPO, "include", "q2048.h")) as fh:
        header = fh.read()
    for path in (N.LIB_PATH, N.HOST_LIB_PATH):
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
        assert {n for n in exported if n.startswith("q2048_nts_")} == set(NAMES), path
    assert {n for n in N._SIGNATURES if n.startswith("q2048_nts_")} == set(NAMES)
    for name in NAMES:
        assert hasattr(N.host_lib(), name) and hasattr(N.lib(), name), name
        assert f"int {name}(" in header, name
    C = __import__("ctypes")
    for name, plain in (("value", "q2048_nt_value"), ("lookup", "q2048_nt_lookup"), ("choose", "q2048_nt_choose"),
                        ("update", "q2048_nt_update"), ("search_lookup_depth", "q2048_nt_search_lookup_depth")):
        res, args = N._SIGNATURES[plain]                                # `stages` directly after the weights
        assert N._SIGNATURES["q2048_nts_" + name] == (res, [args[0], C.c_uint32] + args[1:]), name
    for name in ("fused_rollout", "play_rollout", "search_play_rollout_depth"):
        res, args = N._SIGNATURES["q2048_nt_" + name]
        assert N._SIGNATURES["q2048_nts_" + name] == (res, args[:3] + [C.c_uint32] + args[3:]), name
    assert N.host_lib().q2048_abi_version() == 7 == N.lib().q2048_abi_version() == N.ABI_VERSION     # the number stays


BAD_SPECS = {"descending": spec(5, 3), "equal": spec(3, 3), "a gap nibble": 0x0300, "a nonzero top nibble": 0x10000003,
             "eight ascending thresholds": 0x87654321, "a zero nibble between nonzero ones": 0x0503}


def entry_calls(L, W=0x1000):
    """name -> call(stages, weights=..., bad=False): every other argument good (made-up aligned addresses), or, with
    `bad`, every other argument wrong in a way that a later check would refuse"""
    a = [0x10000 * (k + 2) for k in range(8)]
    nan = float("nan")

    def mk(fn, good, bad_args, w_pos, s_pos):
        def call(stages, weights=W, bad=False):
            args = list(bad_args if bad else good)
            args[w_pos], args[s_pos] = weights, stages
            return fn(*args)
        return call

    return {
        "value": mk(L.q2048_nts_value, [W, 0, a[0], 64, a[1], None], [W, 0, None, -1, a[1] + 8, None], 0, 1),
        "lookup": mk(L.q2048_nts_lookup, [W, 0, a[0], 64, a[1], None], [W, 0, None, -1, a[1] + 8, None], 0, 1),
        "choose": mk(L.q2048_nts_choose, [W, 0, a[0], 64, 0.3, 7, 50, 3, a[1], None],
                     [W, 0, None, -1, nan, 7, 50, 3, None, None], 0, 1),
        "update": mk(L.q2048_nts_update, [W, 0, a[0], a[1], a[2], a[3], 64, 0.1, 0.97, a[4], None],
                     [W, 0, None, None, a[2] + 8, None, -1, nan, nan, None, None], 0, 1),
        "fused_rollout": mk(L.q2048_nts_fused_rollout, [a[0], a[1], W, 0, 64, 2, 0.3, 0.1, 0.97, 3, 50, 0, None, None, a[2], None],
                            [None, a[1] + 8, W, 0, -1, -1, nan, nan, nan, 3, 50, 0, None, None, None, None], 2, 3),
        "play_rollout": mk(L.q2048_nts_play_rollout, [a[0], a[1], W, 0, 64, 2, 0.0, 3, 50, 0, 0, None, None, a[2], None],
                           [None, a[1] + 8, W, 0, -1, -1, nan, 3, 50, 0, 1 << 8, None, None, None, None], 2, 3),
        "search_lookup_depth": mk(L.q2048_nts_search_lookup_depth, [W, 0, a[0], 64, 1, a[1], a[2], None],
                                  [W, 0, None, -1, 3, a[1] + 8, None, None], 0, 1),
        "search_play_rollout_depth": mk(L.q2048_nts_search_play_rollout_depth,
                                        [a[0], a[1], W, 0, 64, 2, 2, 0.0, 3, 50, 0, 0, None, None, a[2], None],
                                        [None, a[1] + 8, W, 0, -1, -1, 0, nan, 3, 50, 0, 1 << 8, None, None, None, None], 2, 3),
        "promote": mk(L.q2048_nts_promote, [W, 0, 0, 1, None, None], [W, 0, 1, 1, None, None], 0, 1),
    }


@pytest.mark.parametrize("which", ["hip", "host"])
def test_malformed_specs_and_argument_errors(pkg, which):
    """Every malformed spec is Q2048_ERR_RANGE on all nine functions BEFORE any other check: with every other argument
    wrong too (B < 0, NULL and misaligned pointers, a bad depth, bad flags, NaN scalars) and with the weights NULL.  A
    well-formed spec then meets the counterpart's checks in its order.  Made-up addresses: nothing behind them is
    touched, so no device is needed."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    calls = entry_calls(L)
    good_specs = (0, spec(11), spec(3, 6), spec(1, 2, 3, 4, 5, 6, 7), spec(9, 10, 11, 12, 13, 14, 15))
    for name, call in calls.items():
        for what, bad in BAD_SPECS.items():
            assert call(bad) == ERR_RANGE, f"{name}: {what}"
            assert call(bad, bad=True) == ERR_RANGE, f"{name}: {what} before every other check"
            assert call(bad, weights=None, bad=True) == ERR_RANGE, f"{name}: {what} before NULL"
        for good in good_specs:
            if name == "promote":
                continue
            assert call(good, weights=None) == ERR_NULL, f"{name}: spec {good:#x}, NULL weights"
            assert call(good, weights=0x1008) == ERR_ALIGN, f"{name}: spec {good:#x}, misaligned weights"
            assert call(good, bad=True) != ERR_RANGE or name.startswith("search"), name     # (the depth is RANGE as well)
    for name in ("value", "lookup", "choose", "update"):
        assert calls[name](spec(11), bad=True) == ERR_SIZE, name                             # B first, as in q2048_nt_*
    assert calls["search_lookup_depth"](spec(11), bad=True) == ERR_RANGE                     # the depth, then the rest
    # B == 0 and steps == 0 are no-ops behind the checks
    a = 0x20000
    assert L.q2048_nts_value(0x1000, spec(11), a, 0, a, None) == 0 and L.q2048_nts_lookup(0x1000, spec(3, 6), a, 0, a, None) == 0
    assert L.q2048_nts_fused_rollout(a, a, 0x1000, spec(11), 64, 0, 0.3, 0.1, 0.9, 1, 0, 0, None, None, a, None) == 0
    assert L.q2048_nts_play_rollout(a, a, 0x1000, spec(11), 0, 5, 0.0, 1, 0, 0, 0, None, None, a, None) == 0
    assert L.q2048_nts_search_play_rollout_depth(a, a, 0x1000, spec(11), 64, 0, 2, 0.0, 1, 0, 0, 0, None, None, a, None) == 0
    for depth in (0, 3, -1):
        assert L.q2048_nts_search_lookup_depth(0x1000, spec(11), a, 64, depth, a, a, None) == ERR_RANGE
        assert L.q2048_nts_search_play_rollout_depth(a, a, 0x1000, spec(11), 64, 1, depth, 0.0, 1, 0, 0, 0, None, None, a,
                                                     None) == ERR_RANGE
    # promote: the spec, NULL, alignment, then from / to against S
    pr = L.q2048_nts_promote
    assert pr(None, spec(11), 0, 0, None, None) == ERR_NULL and pr(0x1008, spec(11), 0, 0, None, None) == ERR_ALIGN
    for stages, frm, to in ((spec(11), 0, 0), (spec(11), 1, 1), (spec(11), 0, 2), (spec(11), 2, 0), (spec(11), -1, 0),
                            (spec(11), 0, -1), (0, 0, 1), (0, 0, 0), (spec(3, 6), 0, 3), (spec(3, 6), 3, 1)):
        assert pr(0x1000, stages, frm, to, None, None) == ERR_RANGE, (stages, frm, to)


@pytest.mark.parametrize("dev", DEVICES)
def test_refused_calls_write_nothing(pkg, dev):
    """Each entry point refused for a malformed spec, and for its counterpart's LAST check under a good spec, on real
    buffers: weights, boards, aux, outputs, statistics and status keep every byte."""
    L, B, nan = lib(pkg, dev), 64, float("nan")
    W = tables_on(dev, 2)
    boards = t8(dev, K.random_boards(np.random.default_rng(1), B))
    aux = torch.full((B, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    out = torch.full((B * 4 + 8,), 0x6B6B6B6B, dtype=torch.int32, device=dev)
    acts = torch.full((B,), 2, dtype=torch.uint8, device=dev)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    count = torch.full((1,), 0x1234, dtype=torch.int64, device=dev)
    si, sf = torch.full((64,), 7, dtype=torch.int64, device=dev), torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((1,), 0x777, dtype=torch.int32, device=dev)
    everything = (boards, aux, out, acts, done, si, sf, status, count)
    before = [t.clone() for t in everything]
    p = lambda t: t.data_ptr()      # noqa: E731
    g, bad = spec(11), spec(5, 3)
    calls = [
        L.q2048_nts_value(p(W), bad, p(boards), B, p(out), None),
        L.q2048_nts_lookup(p(W), bad, p(boards), B, p(out), None),
        L.q2048_nts_choose(p(W), bad, p(boards), B, 0.3, 1, 0, 0, p(acts), None),
        L.q2048_nts_update(p(W), bad, p(boards), p(acts), p(boards), p(done), B, 0.1, 0.9, p(status), None),
        L.q2048_nts_fused_rollout(p(boards), p(aux), p(W), bad, B, 3, 0.3, 0.1, 0.9, 1, 0, 0, p(si), p(sf), p(status), None),
        L.q2048_nts_play_rollout(p(boards), p(aux), p(W), bad, B, 3, 0.0, 1, 0, 0, 0, p(si), p(sf), p(status), None),
        L.q2048_nts_search_lookup_depth(p(W), bad, p(boards), B, 1, p(out), p(acts), None),
        L.q2048_nts_search_play_rollout_depth(p(boards), p(aux), p(W), bad, B, 3, 2, 0.0, 1, 0, 0, 0, p(si), p(sf), p(status), None),
        L.q2048_nts_promote(p(W), bad, 0, 1, p(count), None),
        L.q2048_nts_promote(p(W), g, 1, 1, p(count), None),
        L.q2048_nts_promote(p(W), g, 0, 2, p(count), None),
    ]
    assert calls == [ERR_RANGE] * len(calls)
    calls = [
        L.q2048_nts_value(p(W), g, p(boards), B, p(out) + 8, None),
        L.q2048_nts_lookup(p(W), g, p(boards), B, p(out) + 8, None),
        L.q2048_nts_choose(p(W), g, p(boards), B, 1.5, 1, 0, 0, p(acts), None),
        L.q2048_nts_update(p(W), g, p(boards), p(acts), p(boards), p(done), B, 0.1, nan, p(status), None),
        L.q2048_nts_fused_rollout(p(boards), p(aux), p(W), g, B, 3, 0.3, nan, 0.9, 1, 0, 0, p(si), p(sf), p(status), None),
        L.q2048_nts_play_rollout(p(boards), p(aux), p(W), g, B, 3, nan, 1, 0, 0, 0, p(si), p(sf), p(status), None),
        L.q2048_nts_play_rollout(p(boards), p(aux), p(W), g, B, 3, 0.0, 1, 0, 0, 1 << 8, p(si), p(sf), p(status), None),
        L.q2048_nts_search_lookup_depth(p(W), g, p(boards), B, 2, p(out) + 8, p(acts), None),
        L.q2048_nts_search_play_rollout_depth(p(boards), p(aux), p(W), g, B, 3, 2, nan, 1, 0, 0, 0, p(si), p(sf), p(status), None),
    ]
    P.sync(dev)
    assert calls == [ERR_ALIGN, ERR_ALIGN, ERR_RANGE, ERR_RANGE, ERR_RANGE, ERR_RANGE, ERR_FLAGS, ERR_ALIGN, ERR_RANGE]
    for t, b in zip(everything, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "a refused call wrote"
    assert_tables_unwritten(dev, 2, "a refused call wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 2. stages == 0 is the plain network; 3. equal tables are invisible to readers
# ---------------------------------------------------------------------------------------------------------------
def _player_state(pkg, dev, B):
    env, _ = AV.midgame_env(pkg, "cpu", B, dead=2)
    return env.boards.numpy().copy(), env.aux.numpy().copy(), env.seed, env.env_id0, env.ctr


def _run_player(call, dev, state, steps):
    boards, aux, seed, id0, ctr = state
    tb, ta = torch.from_numpy(boards.copy()).to(dev), torch.from_numpy(aux.copy()).to(dev)
    si, sf = torch.zeros(64, dtype=torch.int64, device=dev), torch.zeros(16, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    assert call(tb.data_ptr(), ta.data_ptr(), len(boards), steps, seed, id0, ctr & 0xFFFFFFFF, si.data_ptr(), sf.data_ptr(),
                status.data_ptr()) == 0
    P.sync(dev)
    # (the float64 sums are accumulated in an order nobody fixes: compared only through what the boards and counts say)
    return tb.cpu().numpy(), ta.cpu().numpy(), si.cpu().numpy(), int(status.item())


def assert_readers_equal_plain(pkg, O, dev, W, stages, V_plain, what):
    """value, lookup, choose, play_rollout and both search depths of (W, stages) against q2048_nt_* on V_plain"""
    L = lib(pkg, dev)
    rng = np.random.default_rng(65)
    boards = K.random_boards(rng, 65)
    boards[::3] = AV.midgame(O)[0][:22]
    tb = t8(dev, boards)
    assert np.array_equal(nts_value(L, dev, W, stages, boards), NT.nt_value(L, dev, V_plain, boards)[0]), f"{what}: value"
    assert np.array_equal(nts_lookup(L, dev, W, stages, boards), NT.nt_lookup(L, dev, V_plain, boards)[0]), f"{what}: lookup"
    for eps in (0.0, 0.4):
        assert np.array_equal(nts_choose(L, dev, W, stages, boards, eps, 3, 9, 5),
                              NT.nt_choose(L, dev, V_plain, boards, eps, 3, 9, 5)[0]), f"{what}: choose, eps {eps}"
    state = _player_state(pkg, dev, 65)
    for flags, eps in ((0, 0.0), (pkg._native.FLAG_ENV_DQN | pkg._native.FLAG_RESET_SHAPING, 0.2)):
        got = _run_player(lambda b, a, B, n, seed, id0, ctr, si, sf, st: L.q2048_nts_play_rollout(
            b, a, W.data_ptr(), stages, B, n, eps, seed, id0, ctr, flags, si, sf, st, None), dev, state, 40)
        want = _run_player(lambda b, a, B, n, seed, id0, ctr, si, sf, st: L.q2048_nt_play_rollout(
            b, a, V_plain.data_ptr(), B, n, eps, seed, id0, ctr, flags, si, sf, st, None), dev, state, 40)
        for x, y in zip(got, want):
            assert np.array_equal(x, y), f"{what}: play_rollout, flags {flags}"
        assert got[2][pkg._native.ST_EPISODES] > 0
    small = boards[:5]
    ts = t8(dev, small)
    state5 = _player_state(pkg, dev, 5)
    for depth in (1, 2):
        q, legal = nts_search(L, dev, W, stages, small, depth)
        wq = torch.empty((5, 4), dtype=torch.float32, device=dev)
        wl = torch.empty((5,), dtype=torch.uint8, device=dev)
        assert L.q2048_nt_search_lookup_depth(V_plain.data_ptr(), ts.data_ptr(), 5, depth, wq.data_ptr(), wl.data_ptr(),
                                              None) == 0
        P.sync(dev)
        wq, wl = bits(wq), wl.cpu().numpy()
        assert np.array_equal(q, wq) and np.array_equal(legal, wl), f"{what}: search_lookup, depth {depth}"
        steps = 6 if depth == 1 else 2
        got = _run_player(lambda b, a, B, n, seed, id0, ctr, si, sf, st: L.q2048_nts_search_play_rollout_depth(
            b, a, W.data_ptr(), stages, B, n, depth, 0.1, seed, id0, ctr, 0, si, sf, st, None), dev, state5, steps)
        want = _run_player(lambda b, a, B, n, seed, id0, ctr, si, sf, st: L.q2048_nt_search_play_rollout_depth(
            b, a, V_plain.data_ptr(), B, n, depth, 0.1, seed, id0, ctr, 0, si, sf, st, None), dev, state5, steps)
        for x, y in zip(got, want):
            assert np.array_equal(x, y), f"{what}: search_play_rollout, depth {depth}"
    del tb


@pytest.mark.parametrize("dev", DEVICES)
def test_stages_zero_is_the_plain_network(pkg, O, dev):
    """Every nts entry point with stages == 0 gives byte for byte what its nt counterpart gives on the same inputs:
    B = 65 (both search depths: B = 5).  The learners run on two copies of the base values and all 256 MiB are compared."""
    L, V = lib(pkg, dev), NT.base_on(dev)
    assert_readers_equal_plain(pkg, O, dev, V, 0, V, "stages == 0")
    NT.assert_base_unwritten(dev, "a reader wrote the weights")
    B = 65
    s, actions, s2 = NT.nonracing_transitions(O, np.random.default_rng(365), B)
    done = (np.arange(B) % 4 == 0).astype(np.uint8)
    a, b = V.clone(), V.clone()
    ts, ts2, ta, td = t8(dev, s), t8(dev, s2), t8(dev, actions), t8(dev, done)
    st_a, st_b = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    assert L.q2048_nts_update(a.data_ptr(), 0, ts.data_ptr(), ta.data_ptr(), ts2.data_ptr(), td.data_ptr(), B, 0.1, 0.97,
                              st_a.data_ptr(), None) == 0
    assert L.q2048_nt_update(b.data_ptr(), ts.data_ptr(), ta.data_ptr(), ts2.data_ptr(), td.data_ptr(), B, 0.1, 0.97,
                             st_b.data_ptr(), None) == 0
    assert int(st_a.item()) == int(st_b.item()) == BAD_ACTION
    assert_same_bits(a, b, "nts_update at stages == 0")
    assert not np.array_equal(bits(a), bits(V)), "no teeth: nothing was learned"
    # one fused learning step on lanes that cannot race (the boards of test_ntuple), then 20 steps of ONE lane
    for n, steps, boards in ((B, 1, NT.nonracing_boards(pkg, O, NT.base_values(), B, 23, 4000, 0.3)), (1, 20, None)):
        out = []
        for staged in (True, False):
            w = V.clone()
            env = pkg.BatchedGame2048Env(n, seed=23, env_id0=4000, device=dev)
            if boards is not None:
                env.boards.copy_(torch.from_numpy(boards))
            si, sf = torch.zeros(64, dtype=torch.int64, device=dev), torch.zeros(16, dtype=torch.float64, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            head = (env.boards.data_ptr(), env.aux.data_ptr(), w.data_ptr())
            tail = (n, steps, 0.3, 0.1, 0.97, 23, 4000, 0, si.data_ptr(), sf.data_ptr(), status.data_ptr(), None)
            assert (L.q2048_nts_fused_rollout(*head, 0, *tail) if staged else L.q2048_nt_fused_rollout(*head, *tail)) == 0
            P.sync(dev)
            out.append((w, env.boards.cpu(), env.aux.cpu(), si.cpu(), sf.cpu()))
        assert_same_bits(out[0][0], out[1][0], f"nts_fused_rollout at stages == 0, B = {n}")
        assert all(torch.equal(x, y) for x, y in zip(out[0][1:], out[1][1:])), n
        assert not np.array_equal(bits(out[0][0]), bits(V))


@pytest.mark.parametrize("dev", DEVICES)
def test_equal_tables_are_invisible_to_readers(pkg, O, dev):
    """Thresholds (3, 6) and every stage holding the SAME bytes: value, lookup, choose, play_rollout and both search
    depths equal the plain results byte for byte -- whatever table a candidate reads."""
    V = NT.base_on(dev)
    W = torch.stack([V, V, V])
    assert_readers_equal_plain(pkg, O, dev, W, spec(3, 6), V, "three equal tables")
    assert all(np.array_equal(bits(W[k]), bits(NT.base_values())) for k in range(3)), "a reader wrote the weights"


# ---------------------------------------------------------------------------------------------------------------
# 4. crafted boards; 5. random boards
# ---------------------------------------------------------------------------------------------------------------
def crafted(t):
    """Rows for a threshold t (3 <= t <= 15) of an S = 2 spec (t,):
    maxnib exactly t - 1 and exactly t; a state below t where the moves of exactly one axis (left / right) merge two
    t - 1 tiles while up and down keep every tile, so its row mixes two tables; no legal move."""
    lo, hi = t - 1, t
    below = np.array([lo, 1, 2, 1, 2, 1, 2, 1, 1, 2, 1, 2, 0, 0, 0, 0], np.uint8)
    at = below.copy()
    at[0] = hi
    # cells 0, 1 hold t - 1 side by side: left and right merge them (a tile t appears), up / down move without merging
    mix = np.array([lo, lo, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.uint8)
    dead = P.DEAD.numpy().copy()
    return np.stack([below, at, mix, dead])


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", BATCHES)
def test_crafted_boards(pkg, O, dev, B):
    """value, lookup and choose on the crafted rows, tiled to the batch sizes 1 .. 257, for thresholds (t,) with
    t = 3, 11 and 15 (a board holding a 15 cell with t = 15).  The model asserts that the rows really read two tables."""
    L, Vs, W = lib(pkg, dev), tables(2), tables_on(dev, 2)
    for t in (3, 11, 15):
        rows = crafted(t)
        boards = rows[np.arange(B) % len(rows)] if B > 1 else rows[2:3]
        q, legal, moved, cstage = model_eval(O, Vs, (t,), boards)
        if B >= 4:
            assert model_stage(rows, (t,)).tolist()[:2] == [0, 1]
            assert sorted(set(cstage[2].tolist())) == [0, 1], "the merging state mixes two tables in one row"
            assert not legal[3].any()
        else:
            assert sorted(set(cstage[0].tolist())) == [0, 1]
        assert_same_bits(nts_value(L, dev, W, spec(t), boards).view(F32), model_v(Vs, (t,), boards), f"value, t = {t}")
        assert_same_bits(nts_lookup(L, dev, W, spec(t), boards).view(F32), q, f"lookup, t = {t}")
        wrong = NT.model_eval(O, Vs[0], boards)[0]                      # teeth: the plain reading of table 0 differs
        assert not np.array_equal(bits(wrong), bits(q))
        acts, _ = P.model_actions(O, q, mask_of(legal), 3, 9, 5, 0.0)
        assert np.array_equal(nts_choose(L, dev, W, spec(t), boards, 0.0, 3, 9, 5), acts), f"choose, t = {t}"
        acts, explored = P.model_actions(O, q, mask_of(legal), 3, 9, 5, 0.5)
        assert np.array_equal(nts_choose(L, dev, W, spec(t), boards, 0.5, 3, 9, 5), acts), f"exploring choose, t = {t}"
    if B == BATCHES[-1]:
        assert_tables_unwritten(dev, 2, "a reader wrote the weights")


@pytest.mark.parametrize("dev", DEVICES)
def test_three_tables_and_illegal_maxima(pkg, O, dev):
    """S = 3.  The four candidates of ONE state hold at most two different sets of tiles -- both horizontal moves leave
    the same tiles, both vertical moves do, and a move that changes nothing leaves the board -- so one row reads at most
    two tables.  With the thresholds (14, 15) three states read every PAIR of the three: two 8192s merge (stage 0 beside
    1), two 16384s merge (1 beside 2), and two 32768s merge into a 16 cell, which aliases to 0 and takes the largest
    nibble DOWN (stage 2 beside 0).  Then, with the thresholds (5, 10), boards on which an ILLEGAL move holds the
    largest q (found among random boards by the model): the choice is the best LEGAL move."""
    L, Vs, W = lib(pkg, dev), tables(3), tables_on(dev, 3)
    thr = (14, 15)
    pair = lambda hi, lo: np.array([hi, hi, 0, 0, lo, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.uint8)      # noqa: E731
    boards = np.stack([pair(13, 1), pair(14, 1), pair(15, 13)])
    q, legal, moved, cstage = model_eval(O, Vs, thr, boards)
    assert [sorted(set(r.tolist())) for r in cstage] == [[0, 1], [1, 2], [0, 2]] and (moved[2, 0] & 15).max() == 13
    assert_same_bits(nts_lookup(L, dev, W, spec(*thr), boards).view(F32), q, "rows over three tables")
    assert_same_bits(nts_value(L, dev, W, spec(*thr), boards).view(F32), model_v(Vs, thr, boards), "values")
    acts, _ = P.model_actions(O, q, mask_of(legal), 1, 2, 3, 0.0)
    assert np.array_equal(nts_choose(L, dev, W, spec(*thr), boards, 0.0, 1, 2, 3), acts)

    thr = (5, 10)
    pool = capped_boards(np.random.default_rng(34), 20000)
    q, legal, moved, cstage = model_eval(O, Vs, thr, pool)
    masked = np.where(legal, q, -np.inf)
    illegal_max = legal.any(axis=1) & (q.argmax(axis=1) != masked.argmax(axis=1))
    assert illegal_max.sum() >= 32, int(illegal_max.sum())
    boards, q, legal, cstage = pool[illegal_max][:64], q[illegal_max][:64], legal[illegal_max][:64], cstage[illegal_max][:64]
    assert len(np.unique(cstage)) >= 2                                  # (a board with an illegal move is nearly full)
    assert_same_bits(nts_lookup(L, dev, W, spec(*thr), boards).view(F32), q, "rows with an illegal maximum")
    acts, _ = P.model_actions(O, q, mask_of(legal), 1, 2, 3, 0.0)
    got = nts_choose(L, dev, W, spec(*thr), boards, 0.0, 1, 2, 3)
    assert np.array_equal(got, acts) and (got != q.argmax(axis=1)).all()
    assert_tables_unwritten(dev, 3, "a reader wrote the weights")


def capped_boards(rng, B):
    """per board a cap uniform in 1..15, then cells uniform in 0..cap: every stage occurs"""
    cap = rng.integers(1, 16, size=(B, 1))
    return (rng.integers(0, 1 << 30, size=(B, 16)) % (cap + 1)).astype(np.uint8)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("thr", [(8,), (5, 10)])
def test_random_boards_reach_every_stage(pkg, O, dev, thr):
    """4,096 capped random boards: each of the S stages holds at least 5 % of the boards and of the candidates; value,
    lookup and choose equal the model (device == twin == model through the two devices)."""
    S_ = len(thr) + 1
    L, Vs, W = lib(pkg, dev), tables(S_), tables_on(dev, S_)
    key = ("random", thr)
    if key not in _SHARED:
        boards = capped_boards(np.random.default_rng(4096 + S_), 4096)
        q, legal, moved, cstage = model_eval(O, Vs, thr, boards)
        _SHARED[key] = (boards, q, legal, cstage, model_v(Vs, thr, boards))
    boards, q, legal, cstage, v = _SHARED[key]
    for k in range(S_):
        assert (model_stage(boards, thr) == k).mean() >= 0.05 and (cstage == k).mean() >= 0.05, k
    assert (cstage.min(axis=1) != cstage.max(axis=1)).sum() > 20, "rows that mix tables"
    assert_same_bits(nts_value(L, dev, W, spec(*thr), boards).view(F32), v, "values")
    assert_same_bits(nts_lookup(L, dev, W, spec(*thr), boards).view(F32), q, "rows")
    acts, explored = P.model_actions(O, q, mask_of(legal), 7, 100, 2, 0.3)
    assert np.array_equal(nts_choose(L, dev, W, spec(*thr), boards, 0.3, 7, 100, 2), acts) and explored > 0
    assert_tables_unwritten(dev, S_, "a reader wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 6. the TD step where lanes cannot race
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [65, 257])
def test_update_where_lanes_cannot_race(pkg, O, dev, B):
    """test_ntuple's transitions whose lanes share no (p, idx) -- hence no (stage, p, idx) -- with the threshold (15,):
    the crowded boards hold tiles up to 32768, so afterstates fall on both sides.  The sequential staged model is the
    specification; all 512 MiB are compared, writes landed in both stages, and no table but stage(c_act) changed for a
    lane."""
    L, Vs, thr = lib(pkg, dev), tables(2), (15,)
    rng = np.random.default_rng(300 + B)
    s, actions, s2 = NT.nonracing_transitions(O, rng, B)
    assert len(s) == B
    done = (rng.random(B) < 0.3).astype(np.uint8)
    lr, gamma = 0.1, 0.97
    want, want_status, written, wstage = model_update(O, Vs, thr, s, actions, s2, done, lr, gamma)
    wrote = wstage >= 0
    assert want_status == BAD_ACTION and (wstage == 0).sum() >= 5 and (wstage == 1).sum() >= 5
    pp = np.arange(4)[:, None]
    for i in np.flatnonzero(wrote):                                     # only table stage(c_act) changed for a lane
        other = 1 - wstage[i]
        assert np.array_equal(bits(want[other][pp, written[i]]), bits(Vs[other][pp, written[i]]))
        assert not np.array_equal(bits(want[wstage[i]][pp, written[i]]), bits(Vs[wstage[i]][pp, written[i]]))
    plain, _, _ = NT.model_update(O, Vs[0], s, actions, s2, done, lr, gamma)
    assert not np.array_equal(bits(plain), bits(want[0])), "no teeth: the plain step on table 0 gives the same"
    del plain
    W, status = t32(dev, Vs), torch.zeros(1, dtype=torch.int32, device=dev)
    ts, ts2, ta, td = t8(dev, s), t8(dev, s2), t8(dev, actions), t8(dev, done)
    assert L.q2048_nts_update(W.data_ptr(), spec(*thr), ts.data_ptr(), ta.data_ptr(), ts2.data_ptr(), td.data_ptr(), B, lr,
                              gamma, status.data_ptr(), None) == 0
    assert int(status.item()) == want_status
    assert_same_bits(W, want, f"B = {B}")
    for t, a in ((ts, s), (ts2, s2), (ta, actions), (td, done)):
        assert np.array_equal(t.cpu().numpy(), a), "an input was written"


@pytest.mark.parametrize("dev", DEVICES)
def test_fused_one_learning_step(pkg, O, dev):
    """One fused learning step at B = 193 on boards whose lanes cannot race (test_ntuple's search), at epsilon = 1: an exploring
    choice reads no value, so the transitions are those of the plain network and so is the proof that no two lanes
    meet.  The staged model on those transitions is the specification: all 512 MiB, boards, aux and statistics."""
    B, seed, id0, lr, gamma, thr = 193, 23, 4000, 0.1, 0.97, (15,)      # (a B of its own: test_ntuple keeps its boards per B)
    Vs = tables(2)
    boards = NT.nonracing_boards(pkg, O, NT.base_values(), B, seed, id0, 1.0)
    env_loop, st_loop, trans = NT.four_call_run(pkg, O, "cpu", NT.base_values(), B, 1, seed, id0, 1.0, 0.0, gamma,
                                                boards=boards, keep=True)
    s, a, s2, d, _ = trans[0]
    assert not NT.conflicts(NT.entry_sets_many(O, s, a.astype(np.int64), s2, fused=True))
    want, status, written, wstage = model_update(O, Vs, thr, s, a, s2, d, lr, gamma)
    assert status == 0 and (wstage == 0).sum() >= 5 and (wstage == 1).sum() >= 5
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    env.boards.copy_(torch.from_numpy(boards))
    agent = make_agent(pkg, dev, (1 << 15,), 1.0, lr, gamma, seed, id0, weights=t32(dev, Vs))
    agent.fused_rollout(env, 1)
    P.sync(dev)
    assert agent.check_status() == 0
    assert torch.equal(env.boards.cpu(), env_loop.boards.cpu()) and torch.equal(env.aux.cpu(), env_loop.aux.cpu())
    st = agent.stats()
    assert st["steps"] == B and st["valid_moves"] == int((s != s2).any(axis=1).sum())
    assert_same_bits(agent.weights, want, "one fused learning step")


# ---------------------------------------------------------------------------------------------------------------
# 7. one lane, 300 fused steps, S = 3
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_one_lane_300_steps(pkg, O, dev):
    """B = 1 from a reset, thresholds (3, 6) = tiles (8, 64), lr 0.1, gamma 0.97, epsilon 0.3, 300 fused steps in
    launches of 1, 63 and 236 == the four-call loop choose_action (q2048_nts_choose) / env.step / update_q_value
    (q2048_nts_update) / env.reset of a second agent, over all 768 MiB bit for bit, boards, aux and statistics.  The
    lane visits all three stages, and on at least one step the afterstate and the next state's best candidate read
    different tables (by the model's stage function on the loop's transitions)."""
    seed, id0, eps, lr, gamma, cuts, tiles, thr = 5, 77, 0.3, 0.1, 0.97, (1, 63, 236), (8, 64), (3, 6)
    Vs = tables(3)
    env_l = pkg.BatchedGame2048Env(1, seed=seed, env_id0=id0, device=dev)
    loop = make_agent(pkg, dev, tiles, eps, lr, gamma, seed, id0, weights=t32(dev, Vs))
    stages_seen, crossed, episodes, valid = set(), 0, 0, 0
    for _ in range(sum(cuts)):
        s = env_l.boards.cpu().numpy().copy()
        a = loop.choose_action(env_l.boards)
        s2, r, done, _ = env_l.step(a)
        loop.update_q_value(t8(dev, s), a, r, s2, done)
        act, s2n = int(a.cpu().numpy()[0]), s2.cpu().numpy().copy()
        x, _, legal = O.move(s[0], act)
        if legal:
            k = int(model_stage(x[None], thr)[0])
            stages_seen.add(k)
            cs = model_stage(model_moves(O, s2n)[0][0], thr)
            crossed += bool((cs != k).any())
            valid += 1
        episodes += int(done.sum())
        env_l.reset(done)
    assert loop.check_status() == 0
    print(f"stages visited {sorted(stages_seen)}, steps whose next state reads another table {crossed}, episodes {episodes}")
    assert stages_seen == {0, 1, 2} and crossed > 0
    env = pkg.BatchedGame2048Env(1, seed=seed, env_id0=id0, device=dev)
    agent = make_agent(pkg, dev, tiles, eps, lr, gamma, seed, id0, weights=t32(dev, Vs))
    for c in cuts:
        agent.fused_rollout(env, c)
    P.sync(dev)
    assert agent.check_status() == 0
    assert torch.equal(env.boards.cpu(), env_l.boards.cpu()) and torch.equal(env.aux.cpu(), env_l.aux.cpu())
    st = agent.stats()
    assert st["steps"] == 300 and st["episodes"] == episodes and st["valid_moves"] == valid
    assert_same_bits(agent.weights, loop.weights, "300 sequential steps over three tables")
    changed = [int(np.count_nonzero(bits(agent.weights[k]) != bits(Vs[k]))) for k in range(3)]
    assert all(c > 0 for c in changed), changed


# ---------------------------------------------------------------------------------------------------------------
# 8. promotion
# ---------------------------------------------------------------------------------------------------------------
def promotion_indices():
    """flat indices into a stage table [4 * 2^24]: the first and last entry of each pattern, and the neighbours of
    16-byte boundaries"""
    idx = []
    for p in range(4):
        base = p * NIDX
        idx += [base, base + 1, base + 3, base + 4, base + 5, base + 7, base + 8, base + NIDX - 1, base + NIDX - 4,
                base + NIDX - 5, base + 1023, base + 1024, base + 1025, base + (NIDX >> 1) - 1, base + (NIDX >> 1)]
    return np.array(sorted(set(idx)), np.int64)


def model_promote(dst, src):
    d, s = bits(dst).copy(), bits(src)
    copy = (d == 0) & (s != 0)
    d[copy] = s[copy]
    return d.view(F32), int(copy.sum())


@pytest.mark.parametrize("dev", DEVICES)
def test_promotion(pkg, dev):
    """Destination and source crafted at chosen indices -- +0.0, -0.0, ordinary values and NaN against zeros, NaN and
    ordinary values, every combination -- on top of tables that are zero in a third of their entries: all 256 MiB of
    the destination and the count against numpy; the source and the third stage stay untouched; a NULL count pointer
    is accepted; promoting again copies nothing."""
    L = lib(pkg, dev)
    base = bits(NT.base_values()).reshape(-1)
    Vs = np.stack([(base ^ np.uint32(STAGE_XOR[k])).view(F32) for k in range(3)])         # [3, 4 * 2^24], writable
    Vs[0][(base >> 3) % 3 == 0] = 0.0                       # the source: zero in a third of its entries
    Vs[1][(base >> 5) % 3 == 0] = 0.0                       # the destination: zero in another third
    nan, nnan = np.uint32(0x7fc00001), np.uint32(0xffc12345)
    dvals = np.array([0x00000000, 0x80000000, 0x3fc00000, nan], np.uint32)                 # +0.0, -0.0, 1.5, NaN
    svals = np.array([0x00000000, 0x80000000, 0xc0200000, nan, nnan], np.uint32)           # +0.0, -0.0, -2.5, two NaNs
    idx = promotion_indices()
    for n, i in enumerate(idx):
        bits(Vs[1])[i] = dvals[n % 4]
        bits(Vs[0])[i] = svals[(n // 4) % 5]
    combos = {(int(bits(Vs[1])[i]), int(bits(Vs[0])[i])) for i in idx}
    assert len(combos) == 20, "every destination value meets every source value"
    want, n_want = model_promote(Vs[1], Vs[0])
    assert np.isnan(want[idx]).sum() >= 4 and 1 << 20 < n_want < 1 << 26
    W = t32(dev, Vs.reshape(3, 4, NIDX))
    assert np.array_equal(bits(W).reshape(3, -1), bits(Vs)), "the upload keeps NaN payloads and -0.0"
    count = torch.full((1,), -7, dtype=torch.int64, device=dev)
    assert L.q2048_nts_promote(W.data_ptr(), spec(3, 6), 0, 1, count.data_ptr(), None) == 0
    P.sync(dev)
    assert int(count.item()) == n_want
    got = bits(W).reshape(3, -1)
    assert np.array_equal(got[1], bits(want)), "the destination"
    assert np.array_equal(got[0], bits(Vs[0])) and np.array_equal(got[2], bits(Vs[2])), "the source or another stage was written"
    assert L.q2048_nts_promote(W.data_ptr(), spec(3, 6), 0, 1, None, None) == 0              # a NULL count pointer
    assert L.q2048_nts_promote(W.data_ptr(), spec(3, 6), 0, 1, count.data_ptr(), None) == 0
    P.sync(dev)
    assert int(count.item()) == 0 and np.array_equal(bits(W).reshape(3, -1)[1], bits(want)), "a second pass copies nothing"
    # downwards too: from 2 into 0
    want0, n0 = model_promote(Vs[0], Vs[2])
    assert L.q2048_nts_promote(W.data_ptr(), spec(3, 6), 2, 0, count.data_ptr(), None) == 0
    P.sync(dev)
    assert int(count.item()) == n0 and np.array_equal(bits(W).reshape(3, -1)[0], bits(want0))


@pytest.mark.parametrize("dev", DEVICES)
def test_promotion_cascade(pkg, dev):
    """S = 3 through agent.promote(): the pairs (0, 1) then (1, 2), so a stage-0 value reaches stage 2 exactly where
    BOTH upper entries were zero; where stage 1 held a value, stage 2 takes that one."""
    agent = make_agent(pkg, dev, (8, 64))
    assert tuple(agent.weights.shape) == (3, 4, NIDX) and not bool(agent.weights.any())
    w = agent.weights.view(3, -1)
    n = 4 * NIDX
    ids = torch.tensor([0, 5, NIDX - 1, NIDX, 3 * NIDX + 17, n - 1, n - 2, n - 3], device=dev)
    #            stage 0   stage 1   stage 2      -> stage 1, stage 2 afterwards
    rows = [(1.0, 0.0, 0.0, 1.0, 1.0), (2.0, 7.0, 0.0, 7.0, 7.0), (3.0, 0.0, 9.0, 3.0, 9.0), (0.0, 4.0, 0.0, 4.0, 4.0),
            (0.0, 0.0, 6.0, 0.0, 6.0), (5.0, -0.0, 0.0, -0.0, -0.0), (8.0, 0.0, -0.0, 8.0, -0.0), (0.0, 0.0, 0.0, 0.0, 0.0)]
    for i, r in zip(ids.tolist(), rows):
        for k in range(3):
            w[k, i] = r[k]
    counts = agent.promote()
    assert counts == [3, 4], counts            # (0 -> 1): rows 0, 2, 6;  (1 -> 2): rows 0, 1, 3 and 5 (the bits of -0.0 are not zero)
    got = bits(agent.weights).reshape(3, -1)[:, ids.cpu().numpy()]
    want = np.array([[r[0] for r in rows], [r[3] for r in rows], [r[4] for r in rows]], F32)
    assert np.array_equal(got, bits(want)), (got, bits(want))
    assert int(np.count_nonzero(bits(agent.weights))) == int(np.count_nonzero(bits(want)))
    with pytest.raises(ValueError):
        NT.make_agent(pkg, dev).promote()


# ---------------------------------------------------------------------------------------------------------------
# 9. the player and the search
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("profile,rss", [("shaped", False), ("shaped", True), ("nopenalty", False), ("nopenalty", True)])
def test_player_equals_the_four_call_loop(pkg, O, dev, profile, rss):
    """65 mid-game boards with dead boards in front, 200 steps by play_rollout in launches of 1 + 63 + 136 and by the
    four-call loop (q2048_nts_lookup through q_values, legal_moves, env step, env reset) at epsilon 0, thresholds
    (5, 7) = tiles (32, 128): boards, aux, statistics; the weights stay as they were."""
    B, tiles = 65, (32, 128)
    env, dead = AV.midgame_env(pkg, dev, B, profile, rss)
    agent = make_agent(pkg, dev, tiles, weights=tables_on(dev, 3))
    q = agent.q_values(env.boards).cpu().numpy()
    mq, mlegal, _, cstage = model_eval(O, tables(3), (5, 7), env.boards.cpu().numpy())
    assert_same_bits(q, mq, "the row's definition")
    assert len(np.unique(cstage)) == 3, "the start reads all three tables"
    env_loop = P.twin_of(pkg, env)
    for c in P.CUTS:
        agent.play_rollout(env, c)
    st_loop = P.four_call_loop(agent, env_loop, sum(P.CUTS))
    P.sync(dev)
    st = agent.play_stats()
    assert torch.equal(env.boards, env_loop.boards) and torch.equal(env.aux, env_loop.aux)
    assert st["steps"] == st_loop["steps"] == B * sum(P.CUTS) and st["valid_moves"] == st_loop["valid_moves"]
    assert st["episodes"] == st_loop["episodes"] >= B and st["max_tile_hist"] == st_loop["max_tile_hist"]
    assert st["explored"] == 0
    assert_tables_unwritten(dev, 3, "the player wrote to the weights")


@pytest.mark.parametrize("dev", DEVICES)
def test_player_exploration_against_the_model(pkg, O, dev):
    """epsilon = 0.3 against the model of the player's draw contract on the staged model's rows."""
    B, steps, eps, thr = 129, 24, 0.3, (5, 7)
    env, _ = AV.midgame_env(pkg, dev, B, dead=3)
    agent = make_agent(pkg, dev, (32, 128), weights=tables_on(dev, 3))
    model = P.twin_of(pkg, env)
    agent.play_rollout(env, 9, epsilon=eps)
    agent.play_rollout(env, steps - 9, epsilon=eps)
    explored = valid = 0
    for _ in range(steps):
        q, legal, _, _ = model_eval(O, tables(3), thr, model.boards.cpu().numpy())
        acts, e = P.model_actions(O, q, mask_of(legal), model.seed, model.env_id0, model.ctr, eps)
        explored += e
        valid += int(legal.any(axis=1).sum())
        _, _, done, _ = model.step(torch.from_numpy(acts).to(dev))
        model.reset(done)
    P.sync(dev)
    st = agent.play_stats()
    assert torch.equal(env.boards, model.boards) and torch.equal(env.aux, model.aux)
    assert st["explored"] == explored > 0 and st["valid_moves"] == valid and st["steps"] == B * steps


def search_boards(O):
    """Crafted: with t = 2 the spawn of a 4 crosses the threshold (children of one chance node pair read two tables);
    a merge at level two does too (1, 1 side by side after a move).  Then random boards."""
    lone = S.lone_tile(5)                                               # maxnib 1: a spawned 4 (nibble 2) reaches t = 2
    pair = np.array([1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.uint8)   # left: the 2s merge into a 4 at level one
    late = np.array([1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1], np.uint8)   # the 2s can only meet two moves on
    return np.stack([lone, pair, late, S.ONE_MOVE, P.DEAD.numpy(), S.ZERO_BEST])


def search_model(O):
    """The staged model's rows of the crafted boards (thresholds (2,)) and of the random boards (thresholds (5, 10)),
    at both depths, computed once."""
    if "search" not in _SHARED:
        crafted_b = search_boards(O)
        Vs2, Vs3 = tables(2), tables(3)
        with staged_search_model(Vs2, (2,)):
            c1, c2 = S.model_search(O, "nts", crafted_b), SD.model_search2(O, "nts", crafted_b)
            nodes = S.model_nodes(*model_moves(O, crafted_b[:1])[::2])
            kids = model_eval(O, Vs2, (2,), nodes)[3]
            assert {0, 1} <= set(np.unique(kids).tolist()) and (model_stage(nodes, (2,)) == [0, 1] * (len(nodes) // 2)).all()
        rnd = capped_boards(np.random.default_rng(1024), 1024)
        rnd[::5, :6] = 0                                                # room for the spawn
        with staged_search_model(Vs3, (5, 10)):
            r1, r2 = S.model_search(O, "nts", rnd), SD.model_search2(O, "nts", rnd[:128])
        _SHARED["search"] = (crafted_b, c1, c2, rnd, r1, r2)
    return _SHARED["search"]


@pytest.mark.parametrize("dev", DEVICES)
def test_search_rows(pkg, O, dev):
    """search_lookup at depth 1 and 2 against the staged composition of model_search / model_search2: crafted boards
    with t = 2, where a chance node's children cross the threshold, and capped random boards (1,024 at depth 1, 128 at
    depth 2) with the thresholds (5, 10)."""
    L = lib(pkg, dev)
    crafted_b, c1, c2, rnd, r1, r2 = search_model(O)
    Vs2 = tables(2)
    W2, W3 = tables_on(dev, 2), tables_on(dev, 3)
    for depth, want in ((1, c1), (2, c2)):
        q, legal = nts_search(L, dev, W2, spec(2), crafted_b, depth)
        assert_same_bits(q.view(F32), want[0], f"crafted boards, depth {depth}")
        assert np.array_equal(legal, mask_of(want[1]))
    with staged_search_model(Vs2[:1], ()):
        plain = S.model_search(O, "nts", crafted_b)[0]
    assert not np.array_equal(bits(plain), bits(c1[0])), "no teeth: table 0 alone gives the same rows"
    q, legal = nts_search(L, dev, W3, spec(5, 10), rnd, 1)
    assert_same_bits(q.view(F32), r1[0], "1,024 random boards, depth 1")
    assert np.array_equal(legal, mask_of(r1[1]))
    q, legal = nts_search(L, dev, W3, spec(5, 10), rnd[:128], 2)
    assert_same_bits(q.view(F32), r2[0], "128 random boards, depth 2")
    assert np.array_equal(legal, mask_of(r2[1]))
    assert_tables_unwritten(dev, 3, "the search wrote to the weights")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("depth,B", [(1, 1), (1, 3), (1, 4), (1, 5), (2, 1), (2, 2), (2, 3)])
def test_search_batch_edges(pkg, O, dev, depth, B):
    """The ends of a block of four boards (depth 1: a wave per board) and of single blocks (depth 2: a block per
    board): the LAST B of the random boards of test_search_rows' model."""
    _, _, _, rnd, r1, r2 = search_model(O)
    n = 1024 if depth == 1 else 128
    want = (r1 if depth == 1 else r2)[0][n - B:n]
    q, legal = nts_search(lib(pkg, dev), dev, tables_on(dev, 3), spec(5, 10), rnd[n - B:n], depth)
    assert_same_bits(q.view(F32), want, f"depth {depth}, B = {B}")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("depth", [1, 2])
def test_searched_player_against_the_model(pkg, O, dev, depth):
    """8 steps at B = 5 and epsilon 0.2 from crowded boards (the start is built on the CPU twin: both devices play the
    same games): the searched row of the staged model, the player's draw contract, the env's own step and reset."""
    B, steps, eps, thr, tiles = 5, 8, 0.2, (5, 7), (32, 128)
    key = ("searched player", depth)
    if key not in _SHARED:
        start, _ = AV.midgame_env(pkg, "cpu", B, dead=1)
        sd = start.state_dict()
        model = P.twin_of(pkg, start)
        explored = 0
        with staged_search_model(tables(3), thr):
            for _ in range(steps):
                boards = model.boards.numpy()
                q, legal = (S.model_search(O, "nts", boards) if depth == 1 else SD.model_search2(O, "nts", boards))[:2]
                acts, e = P.model_actions(O, q, mask_of(legal), model.seed, model.env_id0, model.ctr, eps)
                explored += e
                _, _, done, _ = model.step(torch.from_numpy(acts))
                model.reset(done)
        _SHARED[key] = (sd, model.boards.clone(), model.aux.clone(), explored)
    sd, boards, aux, explored = _SHARED[key]
    env = P.make_env(pkg, dev, B)
    env.load_state_dict(sd)
    agent = make_agent(pkg, dev, tiles, weights=tables_on(dev, 3))
    agent.search_rollout(env, 3, epsilon=eps, depth=depth)
    agent.search_rollout(env, steps - 3, epsilon=eps, depth=depth)
    P.sync(dev)
    assert torch.equal(env.boards.cpu(), boards) and torch.equal(env.aux.cpu(), aux)
    st = agent.play_stats()
    assert st["steps"] == B * steps and st["explored"] == explored
    q, legal = agent.search_lookup(env.boards, depth=depth)
    assert q.shape == (B, 4) and legal.shape == (B,) and q.device == env.boards.device


# ---------------------------------------------------------------------------------------------------------------
# 10. racing learning by properties
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_racing_learning_at_65536_boards_properties(pkg, O, dev):
    """65,536 lanes, epsilon = 1, 4 steps in launches of 1 + 3 from a reset, thresholds (2, 11) = tiles (4, 2048): an
    exploring choice reads no value, so the trajectories equal those of the four-call loop.  The weights sit between
    two guard regions: no write lands outside [S, 4, 2^24].  Stage 2 -- no board reaches a 2048 in four steps -- is
    unchanged; stages 0 and 1 change, at visited (stage, p, idx) only; the values stay finite; the statistics count
    every step, valid move and exploration."""
    B, steps, seed, tiles, thr = 65536, 4, 31, (4, 2048), (2, 11)
    guard, n = 4096, 3 * 4 * NIDX
    flat = torch.zeros(n + 2 * guard, dtype=torch.float32, device=dev)
    flat[:guard] = 12345.0
    flat[-guard:] = 12345.0
    W = flat[guard:guard + n].view(3, 4, NIDX)
    W[2] = tables_on(dev, 3)[2]
    assert W.data_ptr() % 16 == 0
    env = pkg.BatchedGame2048Env(B, seed=seed, device=dev)
    agent = make_agent(pkg, dev, tiles, eps=1.0, lr=0.05, gamma=0.9, seed=seed, id0=0, weights=W)
    agent.fused_rollout(env, 1)
    agent.fused_rollout(env, steps - 1)
    loop_env = pkg.BatchedGame2048Env(B, seed=seed, device=dev)
    loop = make_agent(pkg, dev, tiles, eps=1.0, lr=0.05, gamma=0.9, seed=seed, id0=0, weights=W)
    visited = np.zeros((2, 4 * NIDX), bool)
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
        x = moved[np.arange(B), a][took]
        k = model_stage(x, thr)
        assert k.max() <= 1
        for stage in (0, 1):
            visited[stage][NT.entry_ids(x[k == stage]).ravel()] = True
        loop_env.reset(done)
    P.sync(dev)
    assert torch.equal(env.boards, loop_env.boards) and torch.equal(env.aux, loop_env.aux)
    st = agent.stats()
    assert st["steps"] == B * steps and st["valid_moves"] == valid and st["explored"] == explored == valid
    assert bool((flat[:guard] == 12345.0).all()) and bool((flat[-guard:] == 12345.0).all()), "a write outside the tables"
    assert np.array_equal(bits(W[2]), bits(tables(3)[2])), "the table no board could reach was written"
    for stage in (0, 1):
        v = W[stage].cpu().numpy().ravel()
        changed = np.flatnonzero(v)
        assert np.isfinite(v[changed]).all() and np.abs(v[changed]).max() < 1e4
        assert len(changed) and visited[stage][changed].all(), f"stage {stage}: an entry no lane visited was written"
        assert len(changed) > int(visited[stage].sum()) // 2
    assert agent.check_status() == 0
