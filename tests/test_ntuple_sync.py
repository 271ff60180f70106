"""The synchronous batch step of the 6-tuple afterstate network (q2048_nt_sync_update, q2048_nt_sync_fused_rollout):
V = float32 [4, 2^24] beside caller-owned accumulators uint64 [4, 2^24, 2] = {S, C} and, for the fused learner, a
scratch word per lane, against a numpy model that applies the contract of include/q2048.h literally -- errors on the
frozen V, quantised, summed per occurrence with np.add.at in int64, then ONE write per touched weight -- and
BatchedNTupleAgent(synchronous=True).  (The scripts: test_ntuple_sync_scripts.py.)

Which test executes which kernel (device) / function (CPU twin):
  k_nt_sync_update_acc + k_nt_sync_apply   test_update_where_lanes_collide, test_permutation, test_quantisation_edges,
                                           the loops of test_fused_is_the_four_call_loop_and_the_model
  k_nt_sync_step + k_nt_sync_apply         test_fused_is_the_four_call_loop_and_the_model, test_splits,
                                           test_device_equals_cpu_twin, test_reproducible_at_the_racing_size,
                                           test_learning_rate_zero, the agent tests
  the argument checks                      test_abi, test_argument_errors_need_no_device, test_refused_calls_write_nothing

Every comparison of V is over all 256 MiB as float32 bit patterns, acc and pend are compared as "all zero", boards, aux
and the integer statistics exactly.  There is no tolerance but on the float statistics (an atomic float sum on the
device: 1e-9 relative, as in test_ntuple_lambda).  Nothing needs one: q is an integer, S and C are integer sums below
2^53, m is one float64 division, d one float64 product rounded once to float32, the write one float32 addition."""
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
base_values = NT.base_values
NAMES = ("q2048_nt_sync_update", "q2048_nt_sync_fused_rollout")
ACC_SHAPE = (4, NIDX, 2)
KBLOCK = 256                                      # lanes per block of the device kernels
CLAMP, SCALE = 262144.0, 4096.0
_SHARED = {}


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def model_quantise(err):
    """q = isnan(err) ? 0 : llrint(clamp(err, -2^18, 2^18) * 2^12): np.rint rounds to nearest even -> int64"""
    err = np.asarray(err, np.float64)
    q = np.rint(np.clip(np.where(np.isnan(err), 0.0, err), -CLAMP, CLAMP) * SCALE)
    return q.astype(np.int64)


def model_sync_update(O, V, s, actions, s2, done, lr, gamma, inplace=False):
    """Phase A on the frozen V, phase B once per touched weight.
    -> (values, status word, {"q": int64 per contributing lane, "ids": their entry ids [n, 32], "S", "C", "uniq"})"""
    s, s2 = np.asarray(s, np.uint8).reshape(-1, 16), np.asarray(s2, np.uint8).reshape(-1, 16)
    actions, done = np.asarray(actions).astype(np.int64), np.asarray(done).astype(bool)
    B = len(s)
    V = V if inplace else V.copy()
    ok = actions <= 3
    status = 0 if ok.all() else BAD_ACTION
    moved, _, legal = NT.model_moves(O, s)
    act = np.where(ok, actions, 0)
    took = ok & legal[np.arange(B), act]
    info = {"took": took}
    if not took.any():
        return V, status, info
    x = moved[np.arange(B), act][took]
    q2, legal2, _ = NT.model_eval(O, V, s2[took])
    live = (~done[took]) & legal2.any(axis=1)
    target = (gamma * NT.model_best(q2, legal2).astype(np.float64)) * live.astype(np.float64)
    with np.errstate(invalid="ignore"):
        err = target - NT.model_v(V, x).astype(np.float64)
    q = model_quantise(err)
    ids = NT.entry_ids(x)                                            # [n, 32], p * 2^24 + idx, per occurrence
    uniq, inv = np.unique(ids.ravel(), return_inverse=True)
    S, C = np.zeros(len(uniq), np.int64), np.zeros(len(uniq), np.int64)
    np.add.at(S, inv, np.repeat(q, 32))
    np.add.at(C, inv, 1)
    m = S.astype(np.float64) / (C.astype(np.float64) * SCALE)
    d = ((lr * 0.03125) * m).astype(F32)
    flat = V.reshape(-1)
    flat[uniq] = flat[uniq] + d
    info.update(q=q, ids=ids, S=S, C=C, uniq=uniq, err=err, x=x)
    return V, status, info


# ---------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------
def acc_on(dev):
    """The accumulators, 1 GiB of zeros, allocated once per device: every call leaves them all zero (asserted)."""
    key = ("acc", str(dev))
    if key not in _SHARED:
        _SHARED[key] = torch.zeros(ACC_SHAPE, dtype=torch.int64, device=dev)
    return _SHARED[key]


def assert_all_zero(t, what):
    assert int(torch.count_nonzero(t)) == 0, what


def sync_update(L, dev, weights, s, actions, s2, done, lr, gamma):
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ts, ts2, ta, td = t8(dev, s), t8(dev, s2), t8(dev, actions), t8(dev, done)
    acc = acc_on(dev)
    assert L.q2048_nt_sync_update(weights.data_ptr(), acc.data_ptr(), ts.data_ptr(), ta.data_ptr(), ts2.data_ptr(),
                                  td.data_ptr(), len(s), lr, gamma, status.data_ptr(), None) == 0
    P.sync(dev)
    for t, a in ((ts, s), (ts2, s2), (ta, actions), (td, done)):
        assert np.array_equal(t.cpu().numpy(), a), "an input was written"
    assert_all_zero(acc, "acc is not all zero after the call")
    return int(status.item())


def make_agent(pkg, dev, eps=0.3, lr=0.1, gamma=0.95, seed=P.SEED, id0=P.ID0, epochs=100, synchronous=True):
    kw = {"synchronous": True} if synchronous else {}
    return pkg.BatchedNTupleAgent(epochs, learning_rate=lr, discount_factor=gamma, exploration_rate=eps, seed=seed,
                                  env_id0=id0, device=dev, **kw)


def fused_run(pkg, dev, V, B, launches, seed, id0, eps, lr, gamma, synchronous=True, boards=None):
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    agent = make_agent(pkg, dev, eps, lr, gamma, seed, id0, synchronous=synchronous)
    agent.weights.copy_(t32("cpu", V))
    if boards is not None:
        env.boards.copy_(torch.from_numpy(boards))
    for k in launches:
        agent.fused_rollout(env, k)
    P.sync(dev)
    assert agent.check_status() == 0
    if synchronous:
        assert_all_zero(agent.sync_acc, "acc is not all zero after the launches")
        assert_all_zero(agent.sync_pend, "pend is not all zero after the launches")
    return env, agent


def assert_same_state(a, b, what):
    """(env, agent) pairs: V, boards, aux and the integer statistics exactly"""
    (env_a, ag_a), (env_b, ag_b) = a, b
    assert torch.equal(env_a.boards.cpu(), env_b.boards.cpu()), f"{what}: boards differ"
    assert torch.equal(env_a.aux.cpu(), env_b.aux.cpu()), f"{what}: aux records differ"
    assert torch.equal(ag_a.stats_i.cpu(), ag_b.stats_i.cpu()), f"{what}: integer statistics differ"
    assert torch.allclose(ag_a.stats_f.cpu(), ag_b.stats_f.cpu(), rtol=1e-9, atol=0.0), f"{what}: float statistics differ"
    assert_same_bits(ag_a.weights, bits(ag_b.weights).view(F32), what)


def up_down_symmetric(rng, n):
    """Boards [r0, r1, r1, r0] whose rows have an empty first cell: a left move changes them and keeps the mirror, so
    every entry of the afterstate occurs at least twice among its 32."""
    rows = rng.integers(1, 12, size=(n, 2, 4), dtype=np.uint8)
    rows[:, :, 0] = 0
    return np.concatenate([rows[:, 0], rows[:, 1], rows[:, 1], rows[:, 0]], axis=1)


def colliding_batch(O, kind, B):
    """(s, actions, s2, done) of B lanes whose afterstates collide in the way `kind` says."""
    key = (kind, B)
    if key in _SHARED:
        return _SHARED[key]
    rng = np.random.default_rng(1000 + B)
    pool = AV.crowded()
    dead = P.DEAD.numpy()
    if kind == "one afterstate":                  # every lane learns on the same x; s2 (so the error) differs
        s = np.repeat(pool[77][None], B, axis=0)
        actions = np.full(B, 0, np.uint8)
        x = O.move(s[0], 0)[0]
        assert O.move(s[0], 0)[2]
        s2 = np.stack([dead.copy() if i % 9 == 4 else AV.spawned(rng, x) for i in range(B)])
        done = (np.arange(B) % 5 == 1).astype(np.uint8)
    elif kind == "shared patterns":               # rows 0 and 1 are one pair for all lanes, rows 2 and 3 each lane's own:
        s = pool[rng.permutation(len(pool))[:B]].copy()           # a left move keeps rows apart, so P0 and P2 of image 0 collide
        s[:, :8] = np.array([0, 3, 4, 5, 2, 0, 6, 7], np.uint8)
        actions = np.zeros(B, np.uint8)
        s2 = np.stack([AV.spawned(rng, O.move(b, 0)[0]) for b in s])
        done = (rng.random(B) < 0.2).astype(np.uint8)
    elif kind == "symmetric":                     # every afterstate has a mirror; the board with one tile is lane 0 and 1
        s = up_down_symmetric(rng, B)
        s[0] = 0
        s[0, 3] = 1                               # one tile: left puts it into the corner (the transpose's fixed point)
        s[1] = s[0]
        s[2::8] = s[2]                            # and symmetric boards that several lanes share
        actions = np.zeros(B, np.uint8)
        s2 = np.stack([AV.spawned(rng, O.move(b, 0)[0]) for b in s])
        done = (rng.random(B) < 0.2).astype(np.uint8)
    else:                                         # "mixed": bad actions, unchanged boards, done lanes and dead s' among
        assert kind == "mixed"                    # lanes of all three kinds above
        parts = [colliding_batch(O, k, B) for k in ("one afterstate", "shared patterns", "symmetric")]
        pick = rng.integers(0, 3, size=B)
        s = np.stack([parts[pick[i]][0][i] for i in range(B)])
        actions = np.array([parts[pick[i]][1][i] for i in range(B)], np.uint8)
        s2 = np.stack([parts[pick[i]][2][i] for i in range(B)])
        done = np.array([parts[pick[i]][3][i] for i in range(B)], np.uint8)
        actions[3::7] = 7                                                    # a bad action
        for i in range(5, B, 11):                                            # an action that does not change s
            s[i], actions[i] = P.one_move_board(i % 4), (i + 1) % 4
            s2[i] = s[i]
        s2[2::5] = dead
    _SHARED[key] = (s, actions, s2, done)
    return _SHARED[key]


# ---------------------------------------------------------------------------------------------------------------
# 1. q2048_nt_sync_update against the model where lanes collide
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("kind", ["one afterstate", "shared patterns", "symmetric", "mixed"])
@pytest.mark.parametrize("B", [63, 64, 65, KBLOCK - 1, KBLOCK, KBLOCK + 1])
def test_update_where_lanes_collide(pkg, O, dev, kind, B):
    """B at the ends of a wave and of a block.  The model is the specification BECAUSE lanes collide: the sums are
    integers.  Asserted of each batch, from the model's own sums, that it collides the way its name says."""
    L, V = lib(pkg, dev), base_values()
    s, actions, s2, done = colliding_batch(O, kind, B)
    lr, gamma = 0.1, 0.97
    want, want_status, info = model_sync_update(O, V, s, actions, s2, done, lr, gamma)
    n, C, ids = int(info["took"].sum()), info["C"], info["ids"]
    per_lane_distinct = np.array([len(set(r.tolist())) for r in ids])
    if kind == "one afterstate":
        assert n == B and C.min() == B and len(set(info["q"].tolist())) > 3
    elif kind == "shared patterns":
        assert n == B and (C == B).any() and (C == 1).sum() > 8 * B
    elif kind == "symmetric":
        assert n == B and (per_lane_distinct <= 16).all() and per_lane_distinct[0] < 16 and C.max() > 4
    else:
        took = info["took"]
        assert want_status == BAD_ACTION and (~took & (actions <= 3)).any() and (took & (done == 1)).any()
        assert (took & (s2 == P.DEAD.numpy()).all(axis=1)).any() and C.max() > 8 and (C == 1).any()
    assert np.count_nonzero(bits(want) != bits(V)) > len(info["uniq"]) // 2

    weights = t32(dev, V)
    assert sync_update(L, dev, weights, s, actions, s2, done, lr, gamma) == want_status
    assert_same_bits(weights, want, f"{kind}, B = {B}")


# ---------------------------------------------------------------------------------------------------------------
# 2. the order of the lanes does not show
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_permutation(pkg, O, dev):
    """B = 4097 samples that collide heavily (sixteen copies of the mixed batch, each with spawns of its own in s'), and
    the same samples in another lane order: the same bytes in all of V."""
    L, V, B = lib(pkg, dev), base_values(), 4097
    rng = np.random.default_rng(4097)
    mixed = colliding_batch(O, "mixed", KBLOCK + 1)
    s, actions, s2, done = (np.concatenate([part] * 16)[:B] for part in mixed)
    assert len(s) == B
    s2 = np.stack([AV.spawned(rng, b) if i % 3 else b for i, b in enumerate(s2)])       # the errors of equal samples differ
    first = t32(dev, V)
    status = sync_update(L, dev, first, s, actions, s2, done, 0.1, 0.97)
    order = rng.permutation(B)
    second = t32(dev, V)
    assert sync_update(L, dev, second, s[order], actions[order], s2[order], done[order], 0.1, 0.97) == status == BAD_ACTION
    changed = np.count_nonzero(bits(first) != bits(V))
    assert changed > 1000
    assert_same_bits(second, bits(first).view(F32), "another lane order")


# ---------------------------------------------------------------------------------------------------------------
# 3. the edges of the quantisation
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_quantisation_edges(pkg, O, dev):
    """On a V prepared so that they occur, and checked from first principles beside the model.  All samples are done
    (target 0), so err = -v(x); x_i is the afterstate of lane i, no two lanes share an entry unless said.
      lanes 0, 1   v(x) = -/+ 1e6: err clamps to +/- 262144, the weights move by (float)((lr / 32) * +/-262144)
      lanes 2, 3   err = (2 + 1/2) * 2^-12 and (3 + 1/2) * 2^-12: ties on the grid, rounded to even: q = 2 and q = 4
      lanes 4, 5   share rows 0 and 1; an entry only lane 4 reads is NaN: its error contributes 0 but counts, so the
                   weights both read move by HALF of lane 5's error, the weights only lane 5 reads by all of it"""
    L, lr = lib(pkg, dev), 0.1
    pool = AV.crowded()
    s = np.stack([b for b in pool[:40] if O.move(b, 0)[2]][:6])       # a left move changes each of them
    s[4, :8] = s[5, :8] = np.array([0, 3, 4, 5, 2, 0, 6, 7], np.uint8)
    actions, done = np.zeros(6, np.uint8), np.ones(6, np.uint8)
    x = np.stack([O.move(b, 0)[0] for b in s])
    assert all(O.move(b, 0)[2] for b in s)
    ids = NT.entry_ids(x)
    assert all(len(set(r.tolist())) == 32 for r in ids)
    for i in range(6):
        for j in range(i + 1, 6):
            assert (i, j) == (4, 5) or not set(ids[i].tolist()) & set(ids[j].tolist())
    shared = sorted(set(ids[4].tolist()) & set(ids[5].tolist()))
    only5 = sorted(set(ids[5].tolist()) - set(shared))
    nan_id = ids[4][8]                                                  # pattern 1, image 0: it reads rows 1 and 2
    assert shared and only5 and nan_id not in shared
    V = np.zeros((4, NIDX), F32)
    flat = V.reshape(-1)
    flat[ids[0][0]], flat[ids[1][0]] = F32(-1e6), F32(1e6)
    flat[ids[2][0]], flat[ids[3][0]] = F32(-2.5 / 4096), F32(-3.5 / 4096)
    flat[nan_id] = F32(np.nan)
    flat[only5[0]] = F32(-0.75)                                         # lane 5: err = 0.75, q = 3072
    want, _, info = model_sync_update(O, V, s, actions, x, done, lr, 0.97)
    assert info["q"].tolist() == [1 << 30, -(1 << 30), 2, 4, 0, 3072]
    step = lambda q, c=1: F32((lr * 0.03125) * (q / (c * 4096.0)))      # noqa: E731
    w = want.reshape(-1)
    assert w[ids[0][1]] == step(1 << 30) == F32(lr * 0.03125 * 262144.0) and w[ids[1][1]] == -w[ids[0][1]]
    assert w[ids[2][1]] == step(2) and w[ids[3][1]] == step(4) and step(4) != step(3)
    assert all(w[i] == step(3072, 2) for i in shared) and w[only5[1]] == step(3072) and np.isnan(w[nan_id])
    assert all(bits(w[i:i + 1])[0] == 0 for i in ids[4] if i not in shared and i != nan_id), "d = +0.0 was not added"

    weights = t32(dev, V)
    assert sync_update(L, dev, weights, s, actions, x, done, lr, 0.97) == 0
    assert_same_bits(weights, want, "quantisation edges")


# ---------------------------------------------------------------------------------------------------------------
# 4. the fused learner is the four-call loop is the model
# ---------------------------------------------------------------------------------------------------------------
def loop_run(pkg, O, dev, V, B, steps, seed, id0, eps, lr, gamma):
    """choose_action -> env.step -> update_q_value (q2048_nt_sync_update) -> env.reset(done), `steps` times, and the
    model on the same transitions, step after step on `want`.
    -> (env, agent, the statistics the fused learner counts, want)"""
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    agent = make_agent(pkg, dev, eps, lr, gamma, seed, id0)
    agent.weights.copy_(t32("cpu", V))
    want = V.copy()
    thr = 0 if eps <= 0.0 else int(np.ceil(eps * 4294967296.0))
    st = {"steps": 0, "episodes": 0, "valid_moves": 0, "explored": 0, "score_sum": 0}
    touched = 0
    for t in range(steps):
        s_dev = env.boards.clone()
        s = s_dev.cpu().numpy().copy()
        has_move = env.legal_moves().cpu().numpy() != 0
        actions = agent.choose_action(env.boards)
        s2, reward, done, _ = env.step(actions)
        agent.update_q_value(s_dev, actions, reward, s2, done)
        s2, a, d = s2.cpu().numpy().copy(), actions.cpu().numpy(), done.cpu().numpy().copy()
        st["steps"] += B
        st["episodes"] += int(d.sum())
        st["valid_moves"] += int((s != s2).any(axis=1).sum())
        st["score_sum"] += int(env.score.cpu().numpy()[d].sum())
        st["explored"] += sum(int(O.draws(seed, id0 + i, t)[0]) < thr and bool(has_move[i]) for i in range(B))
        _, _, info = model_sync_update(O, want, s, a, s2, d, lr, gamma, inplace=True)
        touched += len(info.get("uniq", ()))
        env.reset(done)
    P.sync(dev)
    assert agent.check_status() == 0
    assert_all_zero(agent.sync_acc, "acc is not all zero after the loop")
    return env, agent, st, want, touched


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B,launches", [(1, (1, 63, 236)), (257, (1, 26, 13))])
def test_fused_is_the_four_call_loop_and_the_model(pkg, O, dev, B, launches):
    """From the base values at epsilon 0.3, lr 0.1, gamma 0.97: B = 1 for 300 steps (the lane reads its own earlier
    writes on every step), B = 257 for 40 steps (colliding lanes: fresh games share most of their entries), each in
    several launches.  The loop's weights and the fused learner's are the model's, all 256 MiB; boards, aux and the
    statistics are the loop's."""
    seed, id0, eps, lr, gamma = 5, 77, 0.3, 0.1, 0.97
    env_loop, agent_loop, st_loop, want, touched = loop_run(pkg, O, dev, base_values(), B, sum(launches), seed, id0, eps,
                                                            lr, gamma)
    assert st_loop["episodes"] > 0 or B == 257
    assert touched > 16 * sum(launches) and 0 < st_loop["explored"] < st_loop["steps"]
    assert_same_bits(agent_loop.weights, want, f"the four-call loop, B = {B}")
    env, agent = fused_run(pkg, dev, base_values(), B, launches, seed, id0, eps, lr, gamma)
    LT.assert_same_run(env, agent, env_loop, st_loop, f"B = {B}")
    assert_same_bits(agent.weights, want, f"the fused learner, B = {B}")


# ---------------------------------------------------------------------------------------------------------------
# 5. splits, 6. device and CPU twin, 7. the racing size, 8. lr = 0
# ---------------------------------------------------------------------------------------------------------------
def reference_4096(pkg, dev):
    """16 steps at B = 4096 in one call from the base values: the run tests 5 and 6 compare with, once per device"""
    key = ("ref4096", str(dev))
    if key not in _SHARED:
        _SHARED[key] = fused_run(pkg, dev, base_values(), 4096, (16,), 9, 3000, 0.2, 0.1, 0.97)
    return _SHARED[key]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("launches", [(1,) * 16, (5, 11)])
def test_splits(pkg, dev, launches):
    """16 steps in one call == 16 calls of one step == 5 + 11, at B = 4096"""
    whole = reference_4096(pkg, dev)
    assert np.count_nonzero(bits(whole[1].weights) != bits(base_values())) > 1000
    split = fused_run(pkg, dev, base_values(), 4096, launches, 9, 3000, 0.2, 0.1, 0.97)
    assert_same_state(split, whole, f"launches {launches}")


@pytest.mark.gpu
def test_device_equals_cpu_twin(pkg, monkeypatch):
    """B = 4096, 16 steps: V, boards, aux and the integer statistics of the device are the CPU twin's (4 threads), byte
    for byte."""
    monkeypatch.setenv("Q2048_HOST_THREADS", "4")
    twin = fused_run(pkg, "cpu", base_values(), 4096, (16,), 9, 3000, 0.2, 0.1, 0.97)
    assert_same_state(reference_4096(pkg, "cuda:0"), twin, "device against CPU twin")


def test_cpu_twin_does_not_depend_on_its_threads(pkg, monkeypatch):
    """B = 8193 (the twin gives a thread at least 2048 lanes: here up to five ranges), 6 steps, with 1, 4 and 3 threads:
    the same bytes"""
    run = lambda: fused_run(pkg, "cpu", base_values(), 8193, (2, 4), 9, 3000, 0.2, 0.1, 0.97)      # noqa: E731
    monkeypatch.setenv("Q2048_HOST_THREADS", "1")
    one = run()
    for n in ("4", "3"):
        monkeypatch.setenv("Q2048_HOST_THREADS", n)
        assert_same_state(run(), one, f"{n} threads")


@pytest.mark.parametrize("dev", DEVICES)
def test_reproducible_at_the_racing_size(pkg, dev):
    """B = 65,536, 8 steps, twice from the same bytes: V, boards, aux and the integer statistics are identical.  Beside
    it the same two runs of q2048_nt_fused_rollout, whose lanes race: asserted to be finite, nothing more (a repeat of
    that learner MAY differ; the test does not depend on a race showing up)."""
    B, steps = 65536, 8
    V = base_values()
    runs = [fused_run(pkg, dev, V, B, (steps,), 13, 0, 0.1, 0.1, 0.97) for _ in range(2)]
    assert_same_state(runs[0], runs[1], "the repeat")
    assert np.count_nonzero(bits(runs[0][1].weights) != bits(V)) > 1000
    assert runs[0][1].stats()["steps"] == B * steps
    del runs
    for _ in range(2):
        _, plain = fused_run(pkg, dev, V, B, (steps,), 13, 0, 0.1, 0.1, 0.97, synchronous=False)
        assert bool(torch.isfinite(plain.weights).all())


@pytest.mark.parametrize("dev", DEVICES)
def test_learning_rate_zero(pkg, dev):
    """lr = 0, B = 4096, 32 steps: boards, aux and the integer statistics are q2048_nt_fused_rollout's with lr = 0, and V
    is equal as values (every touched weight is written as V + 0.0).  From boards a few moves from the end of their games,
    so episodes end and lanes are reset."""
    V, boards = base_values(), np.array(AV.crowded()[:4096])
    env, agent = fused_run(pkg, dev, V, 4096, (32,), 21, 500, 0.3, 0.0, 0.97, boards=boards)
    env_p, plain = fused_run(pkg, dev, V, 4096, (32,), 21, 500, 0.3, 0.0, 0.97, synchronous=False, boards=boards)
    assert torch.equal(env.boards.cpu(), env_p.boards.cpu()) and torch.equal(env.aux.cpu(), env_p.aux.cpu())
    assert torch.equal(agent.stats_i.cpu(), plain.stats_i.cpu()) and agent.stats()["episodes"] > 0
    assert torch.allclose(agent.stats_f.cpu(), plain.stats_f.cpu(), rtol=1e-9, atol=0.0)
    assert np.array_equal(agent.weights.cpu().numpy(), V) and np.array_equal(plain.weights.cpu().numpy(), V)


# ---------------------------------------------------------------------------------------------------------------
# 9. ABI and argument errors
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
    res, args = N._SIGNATURES["q2048_nt_update"]                  # acc after the weights
    assert N._SIGNATURES["q2048_nt_sync_update"] == (res, args[:1] + [C.c_void_p] + args[1:])
    res, args = N._SIGNATURES["q2048_nt_fused_rollout"]           # acc and pend after the weights
    assert N._SIGNATURES["q2048_nt_sync_fused_rollout"] == (res, args[:3] + [C.c_void_p, C.c_void_p] + args[3:])
    assert N.host_lib().q2048_abi_version() == N.lib().q2048_abi_version() == N.ABI_VERSION == 7


def entry_points(L):
    a = [(k + 1) << 32 for k in range(9)]
    nan = float("nan")
    # name: (function, good arguments, required pointers, 16-byte aligned pointers, position of B, {scalar: refused},
    #        positions of weights and acc)
    return {
        "nt_sync_update": (L.q2048_nt_sync_update, [a[0], a[6], a[1], a[2], a[3], a[4], 64, 0.1, 0.97, a[5], None],
                           (0, 1, 2, 3, 4, 5, 9), (0, 1, 2, 4), 6, {7: (nan,), 8: (nan,)}, (0, 1)),
        "nt_sync_fused_rollout": (L.q2048_nt_sync_fused_rollout,
                                  [a[0], a[1], a[2], a[6], a[8], 64, 2, 0.3, 0.1, 0.97, 3, 50, 0, None, None, a[3], None],
                                  (0, 1, 2, 3, 4, 15), (0, 1, 2, 3, 4), 5, {7: (-0.1, 1.5, nan), 8: (nan,), 9: (nan,)},
                                  (2, 3)),
    }


@pytest.mark.parametrize("which", ["hip", "host"])
def test_argument_errors_need_no_device(pkg, which):
    """The order of the q2048_nt_* counterparts -- B, NULL, alignment, (steps,) the scalars -- with acc (then pend)
    directly after the weights in the NULL and in the alignment list; after the alignment, Q2048_ERR_RANGE for
    B > 2^20 and for acc overlapping V: on both libraries, with made-up addresses, so nothing behind them may be
    touched.  B == 0 and steps == 0 are no-ops."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    nan, big = float("nan"), (2 ** 31 - 1) * 256 + 1
    table = entry_points(L)
    for name, (fn, good, pointers, aligned, b_pos, scalars, (w_pos, acc_pos)) in table.items():
        def call(**kw):
            args = list(good)
            for pos, value in kw.items():
                args[int(pos[1:])] = value
            return fn(*args)

        bad_scalar = {f"p{pos}": values[-1] for pos, values in scalars.items()}
        bad_align = {f"p{pos}": good[pos] + 8 for pos in aligned}
        assert acc_pos in pointers and acc_pos in aligned and acc_pos == w_pos + 1
        for value in (-1, big):                                         # B before everything
            assert call(**{f"p{b_pos}": value, f"p{pointers[0]}": None}, **bad_scalar) == ERR_SIZE, name
        for pos in pointers:                                            # NULL before the alignment and the scalars
            kw = {**bad_align, **bad_scalar, f"p{b_pos}": (1 << 20) + 1, f"p{pos}": None}
            assert call(**kw) == ERR_NULL, f"{name}: NULL in position {pos}"
        for pos in aligned:                                             # the alignment before the two range checks
            kw = {**bad_scalar, f"p{b_pos}": (1 << 20) + 1, f"p{pos}": good[pos] + 8}
            assert call(**kw) == ERR_ALIGN, f"{name}: position {pos} off by 8 bytes"
        for pos, values in scalars.items():
            for value in values:
                assert call(**{f"p{pos}": value}) == ERR_RANGE, f"{name}: {value} in position {pos}"
        assert call(**{f"p{b_pos}": (1 << 20) + 1}) == ERR_RANGE, f"{name}: B = 2^20 + 1"
        w = good[w_pos]
        for acc, code in ((w, ERR_RANGE), (w + (1 << 28) - 16, ERR_RANGE), (w - (1 << 30) + 16, ERR_RANGE),
                          (w + (1 << 28), 0), (w - (1 << 30), 0)):      # V is 2^28 bytes, acc 2^30
            assert call(**{f"p{acc_pos}": acc, f"p{b_pos}": 0}) == code, f"{name}: acc at weights {acc - w:+#x}"
        assert call(**{f"p{b_pos}": 0}) == 0, f"{name}: B = 0"
        assert call(**{f"p{b_pos}": 0, f"p{pointers[0]}": None}) == ERR_NULL, f"{name}: B = 0 is checked first"
    fn, good = table["nt_sync_fused_rollout"][:2]
    for steps, eps, code in ((-1, nan, ERR_SIZE), ((1 << 30) + 1, nan, ERR_SIZE), (0, 0.3, 0), (0, nan, ERR_RANGE)):
        args = list(good)
        args[6], args[7] = steps, eps                                   # steps before epsilon
        assert fn(*args) == code, f"nt_sync_fused_rollout: steps = {steps}"
    args = list(good)
    args[3], args[6] = good[2] + 16, -1                                 # the overlap before steps
    assert fn(*args) == ERR_RANGE


@pytest.mark.parametrize("dev", DEVICES)
def test_refused_calls_write_nothing(pkg, dev):
    """Both entry points refused on real buffers -- a NaN lr, a misaligned and a NULL acc, a misaligned and a NULL pend,
    acc inside V, steps < 0 -- : V, boards, aux, pend, statistics and status keep every byte, acc stays zero."""
    L, B = lib(pkg, dev), 64
    nan = float("nan")
    V, acc = NT.base_on(dev), acc_on(dev)
    rng = np.random.default_rng(1)
    boards = t8(dev, NT.K.random_boards(rng, B))
    pend = torch.full((B + 2,), 0x0123456789ABCDE, dtype=torch.int64, device=dev)
    aux = torch.full((B, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    acts = torch.full((B,), 2, dtype=torch.uint8, device=dev)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    si, sf = torch.full((64,), 7, dtype=torch.int64, device=dev), torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((1,), 0x777, dtype=torch.int32, device=dev)
    everything = (boards, pend, aux, acts, done, si, sf, status)
    before = [t.clone() for t in everything]
    p = lambda t: t.data_ptr()      # noqa: E731
    up = lambda a, lr: L.q2048_nt_sync_update(p(V), a, p(boards), p(acts), p(boards), p(done), B, lr, 0.9, p(status), None)  # noqa: E731
    fu = lambda a, pe, lr, steps=3: L.q2048_nt_sync_fused_rollout(p(boards), p(aux), p(V), a, pe, B, steps, 0.3, lr, 0.9, 1,  # noqa: E731
                                                                  0, 0, p(si), p(sf), p(status), None)
    calls = [up(p(acc), nan), up(p(acc) + 8, 0.1), up(None, 0.1), up(p(V) + 4096, 0.1),
             fu(p(acc), p(pend), nan), fu(p(acc) + 8, p(pend), 0.1), fu(None, p(pend), 0.1), fu(p(acc), p(pend) + 8, 0.1),
             fu(p(acc), None, 0.1), fu(p(V) + 4096, p(pend), 0.1), fu(p(acc), p(pend), 0.1, -1)]
    P.sync(dev)
    assert calls == [ERR_RANGE, ERR_ALIGN, ERR_NULL, ERR_RANGE,
                     ERR_RANGE, ERR_ALIGN, ERR_NULL, ERR_ALIGN, ERR_NULL, ERR_RANGE, ERR_SIZE]
    for t, b in zip(everything, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "a refused call wrote"
    NT.assert_base_unwritten(dev, "a refused call wrote the weights")
    assert_all_zero(acc, "a refused call wrote the accumulators")


# ---------------------------------------------------------------------------------------------------------------
# 10. the agent
# ---------------------------------------------------------------------------------------------------------------
def test_constructor_refusals(pkg):
    mk = lambda **kw: pkg.BatchedNTupleAgent(10, device="cpu", **kw)      # noqa: E731
    for kw, word in (({"coherence": True}, "coherence"), ({"stage_tiles": (2048,)}, "stage_tiles"),
                     ({"stage_tiles": (2048,), "carousel": 8}, "stage_tiles"), ({"carousel": 8}, "carousel"),
                     ({"trace_lambda": 0.5}, "trace_lambda"), ({"trace_lambda": 0.0, "trace_depth": 0}, "trace_lambda")):
        with pytest.raises(ValueError, match=word):
            mk(synchronous=True, **kw)
    with pytest.raises(ValueError, match="synchronous"):
        mk(synchronous=1)
    agent = mk(synchronous=True)
    assert agent.sync_acc.shape == ACC_SHAPE and agent.sync_acc.dtype == torch.int64 and agent.sync_pend is None
    assert mk().sync_acc is None and mk().synchronous is False


@pytest.mark.parametrize("dev", DEVICES)
def test_checkpoints_are_the_plain_agents(pkg, dev, tmp_path):
    """A synchronous agent's state_dict has the plain agent's keys (no accumulators, no scratch); each kind loads the
    other's file, bit for bit, and goes on from it: the synchronous agent that loaded the plain file ends where the
    one that never stopped does.  Another B than the first rollout's is refused."""
    seed, id0, B = 3, 40, 64
    env, agent = fused_run(pkg, dev, base_values(), B, (5,), seed, id0, 0.3, 0.1, 0.97)
    sd = agent.state_dict()
    plain = make_agent(pkg, dev, seed=seed, id0=id0, synchronous=False)
    assert set(sd) == set(plain.state_dict()) and not any("sync" in k for k in sd)
    path = os.path.join(tmp_path, "sync.pt")
    torch.save(sd, path)
    plain.load_state_dict(torch.load(path, weights_only=False))
    assert_same_bits(plain.weights, bits(agent.weights).view(F32), "plain <- synchronous")
    torch.save(plain.state_dict(), path)
    again = make_agent(pkg, dev, 0.3, 0.1, 0.97, seed, id0)
    again.load_state_dict(torch.load(path, weights_only=False))
    assert_same_bits(again.weights, bits(agent.weights).view(F32), "synchronous <- plain")
    assert (again.ctr, again.epsilon) == (agent.ctr, agent.epsilon)
    env2 = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    env2.load_state_dict(env.state_dict())
    again.fused_rollout(env2, 7)
    agent.fused_rollout(env, 7)
    P.sync(dev)
    assert torch.equal(env.boards.cpu(), env2.boards.cpu()) and torch.equal(env.aux.cpu(), env2.aux.cpu())
    assert_same_bits(again.weights, bits(agent.weights).view(F32), "after the resume")
    other = pkg.BatchedGame2048Env(B + 1, seed=seed, env_id0=id0, device=dev)
    other.ctr = agent.ctr
    before = bits(agent.weights).copy()
    with pytest.raises(ValueError, match="lanes"):
        agent.fused_rollout(other, 1)
    assert np.array_equal(bits(agent.weights), before)
