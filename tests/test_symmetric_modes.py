"""Every symmetry-folded kernel variant against the numpy model of tests/test_symmetric_table.py.

On the device each (table mode, env profile, workgroup size) of the folded learner is a kernel of its own, and the
folded player and lookup are instantiations of their own; on the CPU twin they are one function with run-time tests.
So every case here runs on both.  The model is the one of test_symmetric_table.py -- np.rot90 / np.fliplr, the nibble
packing, min, a PLAIN agent driven call by call on the canonical boards -- and every comparison is exact.

Which case executes what (table mode of k_fused_rollout with kModeSym; E = env profile):
  Sym+Learn                 test_learner_matrix[strict=False], test_shared_table_values[False], test_big_batch[False]
  Sym+Cas                   test_learner_matrix[strict=True], test_shared_table_values[True], test_big_batch[True]
  Sym+Eval                  test_evaluation_against_numpy, test_episode_log_of_an_evaluation, test_big_batch
  Sym+Frozen                test_closed_key_set_matrix (line_summaries off, plain store)
  Sym+Frozen+Cas            test_closed_key_set_matrix (line_summaries off, strict_td)
  Sym+Frozen+Summary        test_closed_key_set_matrix (line_summaries on, plain store), test_big_batch[False]
  Sym+Frozen+Summary+Cas    test_closed_key_set_matrix (line_summaries on, strict_td), test_big_batch[True]
  E = shaped, DQN, shaped + reset shaping, DQN + reset shaping
                            the four (profile, reset_shaping_state) pairs of test_learner_matrix and of
                            test_player_on_every_profile; shaped and DQN also in test_evaluation_against_numpy
  512 lanes per workgroup   test_big_batch (GPU only); every other case is the 256-lane kernel
  folded k_q_lookup         test_q_values_private_rows (per-env and SINGLE_ENV salts), test_tile_overflow_is_still_reported
  folded k_play_rollout     test_player_on_every_profile"""
import importlib
import math

import numpy as np
import pytest
import torch

from test_symmetric_table import (DEVICES, _quiet, canon, env_rows, frozen_learner, images, legal, make, model_run, pi,
                                  rows_of, same_learner, sync, trained, twin_of, unpack)

PROFILES = [("shaped", False), ("nopenalty", False), ("shaped", True), ("nopenalty", True)]
RECORD = ("env_id", "episode", "action", "reward", "max_log2", "score", "total_return", "q")


def t8(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev)


def bits(t):
    """float32 values as their bit patterns (numpy uint32)."""
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float32)).view(np.uint32)


def drained(log):
    """The device log in the layout of model_run's records, sorted by (env id, episode): reward and return as the
    Python floats of the float32 values (exact), q as four float32 bit patterns."""
    out = [(int(r["env_id"]), int(r["episode"]), int(r["action"]), float(r["reward"]), int(r["max_log2"]),
            int(r["score"]), float(r["total_return"]), tuple(np.asarray(r["q"]).view(np.uint32).tolist()))
           for r in log.drain()]
    return sorted(out)


def assert_same_records(got, want, rows_can_differ):
    """Field for field.  The model's records carry, ninth, g of the board the row belongs to.  So that the frame is
    tested at all, some record must come from a board that is not its own canonical image (g != 0) with an action
    that pi_g moves, and -- `rows_can_differ` -- with a row whose four numbers are not all equal.
    The DQN profile ("nopenalty") ends an episode on an invalid move on a dead board, reward 0.0: the row of that
    board is all zeros before and after the update whatever the kernel does (0 of 118 records of the CPU twin carry a
    reward or a row entry that is not 0.0), so there the row's frame shows only on the "shaped" profile, where the
    final reward is never 0 (112 of 112 rows not constant, 88 of them from a turned board)."""
    assert len(got) == len(want)
    for a, b in zip(got, want):
        for name, x, y in zip(RECORD, a, b):
            assert x == y, (name, a, b)
    moved = [r for r in want if r[8] != 0 and int(pi(r[8], r[2])) != r[2]]
    turned = [r for r in want if r[8] != 0 and len(set(r[7])) > 1]
    print(f"{len(want)} records: {len(moved)} with an action that pi_g moves, {len(turned)} from a turned board with "
          "a row that is not constant")
    assert moved, "no record tests the frame of the action"
    assert turned or not rows_can_differ, "no record tests the permutation of the row"


# ---------------------------------------------------------------------------------------------
# 1 + 4. the folded learner on private rows: table mode x env profile, and its episode log
# ---------------------------------------------------------------------------------------------
B1, STEPS1, EPS1, CUTS1 = 77, 300, 0.3, (1, 63, 236)          # one full wave and a 13-lane tail; the cache hand-over
_learners = {}


def learner_run(pkg, O, dev, profile, rss, strict):
    """The fused folded learner (launches of 1, 63 and 236 steps, an episode log attached) beside the model: a plain
    agent with the same write mode on an env of the same profile, driven by model_run's four calls.  Private rows
    make both a function of their inputs, so a case is run once and shared by the tests below."""
    key = (dev, profile, rss, strict)
    if key not in _learners:
        kw = dict(independent=True, eps=EPS1, cap=18, profile=profile, reset_shaping_state=rss, strict_td=strict)
        env, agent = make(pkg, dev, B1, True, **kw)
        env_m, model = make(pkg, dev, B1, False, **kw)
        log = pkg.EpisodeLog(4096, device=dev)
        for cut in CUTS1:
            agent.fused_rollout(env, cut, episode_log=log)
        records, states = [], []
        explored, episodes = model_run(pkg, O, dev, env_m, model, STEPS1, EPS1, records=records, states=states)
        sync(dev)
        got = drained(log)
        _learners[key] = dict(env=env, agent=agent, env_m=env_m, model=model, log=got, lost=log.lost,
                              records=sorted(records), states=states, explored=explored, episodes=episodes)
    return _learners[key]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("profile,rss", PROFILES)
def test_learner_matrix(pkg, O, dev, profile, rss, strict):
    """What check_fused_equals_model asserts, on every env profile and both write modes.  (shaped, no reset shaping,
    plain store) repeats test_fused_learner_equals_the_model_private_rows[77]: the row that anchors the matrix.
    The CPU twin ends 112 to 118 episodes here; the floor of 64 only proves that the reset path ran."""
    r = learner_run(pkg, O, dev, profile, rss, strict)
    env, agent, env_m, model = r["env"], r["agent"], r["env_m"], r["model"]
    st = agent.stats()
    print(f"{profile} reset_shaping {rss} strict {strict}: rows {st['inserts']} explored {st['explored']} "
          f"episodes {st['episodes']}")
    assert torch.equal(env.boards, env_m.boards), "boards differ"
    assert torch.equal(env.aux, env_m.aux), "aux records differ"
    assert rows_of(agent) == rows_of(model)
    assert st["inserts"] == model.stats()["inserts"] == agent.table_size()
    assert st["explored"] == r["explored"] and st["episodes"] == r["episodes"] and st["steps"] == B1 * STEPS1
    assert st["drops"] == 0 and agent.check_status() == 0 and model.check_status() == 0
    assert r["episodes"] >= 64, "the span must cover the reset path"
    assert not agent.frozen and not model.frozen
    agent.verify_table()


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("profile,rss,strict", [("shaped", False, False), ("nopenalty", True, True)])
def test_episode_log_of_the_learner(pkg, O, dev, profile, rss, strict):
    """rec.action is the ENV's action and rec.q the live row, post-update, in the ENV's frame."""
    r = learner_run(pkg, O, dev, profile, rss, strict)
    assert r["lost"] == 0 and len(r["records"]) == r["episodes"] >= 64
    assert_same_records(r["log"], r["records"], profile == "shaped")


# ---------------------------------------------------------------------------------------------
# 6. q_values on private rows: env `env_id0 + i` and SINGLE_ENV, salted after canonicalisation
# ---------------------------------------------------------------------------------------------
def lookup_pair(dev, agent, reader, boards, env_id=None):
    """(folded q_values of the boards, found) and what they must be: the plain reader's rows of the numpy-canonical
    boards, in the rows of the same env(s), permuted to the boards' frame."""
    cs, g, _ = canon(boards)
    q, found = agent.q_values(t8(dev, boards), env_id=env_id, return_found=True)
    rq, rfound = reader.q_values(t8(dev, cs), env_id=env_id, return_found=True)
    return bits(q), found.cpu().numpy(), env_rows(rq.cpu().numpy(), g).view(np.uint32), rfound.cpu().numpy()


def assert_images_agree(dev, agent, reader, base, env_id=None):
    """The eight images of every board: one row, up to pi_g -- Q(image_g(b))[pi_g(a)] == Q(b)[a]."""
    q0 = bits(agent.q_values(t8(dev, base), env_id=env_id))
    assert (q0 != q0[:, :1]).any(axis=1).sum() > len(base) // 2          # rows that are not constant
    for g, img in enumerate(images(base.reshape(-1, 4, 4))):
        got, found, want, rfound = lookup_pair(dev, agent, reader, np.ascontiguousarray(img).reshape(-1, 16), env_id)
        assert np.array_equal(got, want) and np.array_equal(found, rfound) and found.all(), g
        for a in range(4):
            assert np.array_equal(got[:, int(pi(g, a))], q0[:, a]), (g, a)


@pytest.mark.parametrize("dev", DEVICES)
def test_q_values_private_rows(pkg, O, dev):
    r = learner_run(pkg, O, dev, "shaped", False, False)
    agent, states, id0 = r["agent"], r["states"], r["agent"].env_id0
    _, reader = make(pkg, dev, B1, False, independent=True, cap=18)      # a plain agent reading the same table
    reader.table = agent.table
    # board i in the rows of env id0 + i: the boards step t started from are one visited state per env, in env order
    seen = 0
    for t in range(20, STEPS1, 40):                                     # 7 x 77 = 539 boards
        got, found, want, rfound = lookup_pair(dev, agent, reader, states[t])
        assert np.array_equal(got, want) and np.array_equal(found, rfound) and found.all(), t
        seen += len(got)
    assert seen >= 512
    assert_images_agree(dev, agent, reader, states[150][:64])
    # an env's row is its own: the same boards one env further on are other rows (absent, or other numbers)
    shifted, found_s, want_s, rfound_s = lookup_pair(dev, agent, reader, np.roll(states[150], 1, axis=0))
    assert np.array_equal(shifted, want_s) and np.array_equal(found_s, rfound_s) and not found_s.all()
    # every board in the rows of ONE env: that env's 300 states, then 212 states of the others
    everyone = np.concatenate(states)
    for e in (id0, id0 + B1 - 1):
        own = everyone[e - id0::B1]
        others = np.delete(everyone, np.s_[e - id0::B1], axis=0)[7::97][:212]
        boards = np.concatenate([own, others])
        assert len(own) == STEPS1 and len(boards) == 512
        got, found, want, rfound = lookup_pair(dev, agent, reader, boards, env_id=e)
        assert np.array_equal(got, want) and np.array_equal(found, rfound) and found[:STEPS1].all(), e
        assert not found.all()                                          # (states the env never saw read as absent)
        assert_images_agree(dev, agent, reader, own[100:164], env_id=e)
    assert agent.check_status() == 0


# ---------------------------------------------------------------------------------------------
# 2. the closed key set: write mode x line summaries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_closed_key_set_matrix(pkg, dev):
    """Private rows: no two lanes share an entry, so the compare-and-swap write equals the store, and line summaries
    only shorten the lookup of an absent state -- the four learners are one learner."""
    cases = [(strict, summaries) for strict in (False, True) for summaries in (False, True)]
    learners = {c: frozen_learner(pkg, dev, c[1], strict_td=c[0]) for c in cases}
    env0, first = learners[cases[0]]
    for c in cases[1:]:
        same_learner(env0, first, *learners[c])
    rows = first.table_size()
    with _quiet():
        for env, agent in learners.values():
            agent.fused_rollout(env, 100)
    sync(dev)
    for c in cases[1:]:
        same_learner(env0, first, *learners[c])
    for (strict, summaries), (env, agent) in learners.items():
        st = agent.stats()
        assert st["drops"] > 0 and agent.table_size() == rows and agent.check_status() == 0, (strict, summaries)
        words = agent.table.view(torch.int64).reshape(-1, 4)
        assert agent._summarised == summaries and bool((words[:, 3] != 0).any()) == summaries, (strict, summaries)
        assert agent.frozen and bool(agent.flags & pkg._native.FLAG_TD_CAS) == strict
    print(f"closed key set: {rows} rows, {first.stats()['drops']} drops of {first.stats()['steps']} steps")


# ---------------------------------------------------------------------------------------------
# 3 + 4. evaluation (learn=False) against numpy, and its episode log
# ---------------------------------------------------------------------------------------------
B3, CUTS3, EPS3 = 256, (1, 63, 56), 0.3
_evaluations = {}


def evaluation_run(pkg, O, dev, profile):
    """A folded shared table trained for 200 steps, then three evaluation launches beside the model: per step the
    plain reader's rows of the canonical boards in the env's frame, explore iff x0 < ceil(eps * 2^32) then x1 >> 30
    else the first maximum in the ENV's action order, env.step, reset(done).  A record's q is the STORED row."""
    key = (dev, profile)
    if key in _evaluations:
        return _evaluations[key]
    env, agent = make(pkg, dev, B3, True, cap=16, eps=EPS3, profile=profile)
    with _quiet():
        agent.fused_rollout(env, 200)
    # the carried row a launch leaves in the row cache is what the lane read, and on a SHARED table another lane may
    # have written that row since: the model reads the table, so the evaluation starts from the table too
    agent.invalidate_row_cache()
    sync(dev)
    # An episode of an evaluation ends on a board it has hardly ever seen before, whose stored row is zeros in any
    # frame.  So that the log's rows say something, some envs are put on turned images of dead boards the table HAS
    # a row for (where episodes of the training ended): their first step ends the episode.
    keys, rows = agent.export_rows()
    known = unpack(keys)[(rows != rows[:, :1]).any(axis=1)]
    known = known[legal(pkg, dev, known) == 0][:16]
    for j, b in enumerate(known):
        img = images(b.reshape(1, 4, 4))[1 + j % 7]
        env.boards[j].copy_(t8(dev, img.reshape(-1)))
    model_env = twin_of(pkg, env)
    _, reader = make(pkg, dev, B3, False, cap=16)                        # a plain agent reading the same table
    reader.table = agent.table
    before, st0, rows0 = agent.table.clone(), agent.stats(), agent.table_size()
    agent.status.zero_()
    log = pkg.EpisodeLog(4096, device=dev)
    for k in CUTS3:
        agent.fused_rollout(env, k, learn=False, episode_log=log)
    thr, explored, episodes, records = math.ceil(EPS3 * 4294967296.0), 0, 0, []
    for _ in range(sum(CUTS3)):
        cs, g, _ = canon(model_env.boards.cpu().numpy())
        q = env_rows(reader.q_values(t8(dev, cs)).cpu().numpy(), g)
        acts = np.zeros(B3, dtype=np.uint8)
        for i in range(B3):
            x = O.draws(model_env.seed, model_env.env_id0 + i, model_env.ctr)
            if int(x[0]) < thr:
                acts[i] = int(x[1]) >> 30
                explored += 1
            else:
                acts[i] = int(np.argmax(q[i]))
        _, reward, done, _ = model_env.step(t8(dev, acts))
        over = np.flatnonzero(done.cpu().numpy())
        episodes += len(over)
        aux, rew, mx = model_env.aux_fields(), reward.cpu().numpy(), model_env.max_log2.cpu().numpy()
        for i in over.tolist():
            records.append((model_env.env_id0 + i, int(aux["episode"][i]), int(acts[i]), float(rew[i]), int(mx[i]),
                            int(aux["score"][i]), float(aux["ep_return"][i]), tuple(q[i].view(np.uint32).tolist()),
                            int(g[i])))
        model_env.reset(done)
    sync(dev)
    got = drained(log)
    _evaluations[key] = dict(env=env, agent=agent, model_env=model_env, before=before, st0=st0, rows0=rows0, log=got,
                             lost=log.lost, records=sorted(records), explored=explored, episodes=episodes)
    return _evaluations[key]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("profile", ["shaped", "nopenalty"])
def test_evaluation_against_numpy(pkg, O, dev, profile):
    r = evaluation_run(pkg, O, dev, profile)
    env, agent, st0, st = r["env"], r["agent"], r["st0"], r["agent"].stats()
    print(f"{profile}: explored {r['explored']} episodes {r['episodes']} rows {r['rows0']}")
    assert torch.equal(env.boards, r["model_env"].boards), "boards differ"
    assert torch.equal(env.aux, r["model_env"].aux), "aux records differ"
    assert st["explored"] - st0["explored"] == r["explored"] and st["episodes"] - st0["episodes"] == r["episodes"] > 0
    assert st["steps"] - st0["steps"] == B3 * sum(CUTS3)
    assert torch.equal(agent.table, r["before"]), "an evaluation wrote to the table"
    assert st["inserts"] == st0["inserts"] and st["drops"] == st0["drops"] and agent.table_size() == r["rows0"] > 0
    assert agent.check_status() == 0


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("profile", ["shaped", "nopenalty"])
def test_episode_log_of_an_evaluation(pkg, O, dev, profile):
    r = evaluation_run(pkg, O, dev, profile)
    assert r["lost"] == 0 and len(r["records"]) == r["episodes"] > 0
    assert_same_records(r["log"], r["records"], profile == "shaped")


# ---------------------------------------------------------------------------------------------
# 5. shared table under races: the stored VALUES
# ---------------------------------------------------------------------------------------------
def shared_ledger(O, B, steps, seed, id0):
    """The same games played by the oracle (epsilon 1: the actions are the draws'), as sorted arrays of codes:
    `visited` the canonical keys of every state the reference looked up (s and s', terminal ones included: the keys
    of the oracle agent's dict), `pairs` the (key, pi_g(a)) taken, `triples` the (key, pi_g(a), float32 reward) seen,
    `turned` the pairs reached from a board that is not its own canonical image.  A pair's code is 4 * (index of its
    key in `visited`) + action, a triple's that code above the reward's 32 bits."""
    envs = O.envs_init(B, 4, seed, id0)
    oa = O.Agent(100, 4, 1.0, 0.0, 1.0)
    keys, acts, rews, gs = [], [], [], []
    for t in range(steps):
        _, g, k = canon(envs["board"][:, :16])
        _, _, a, r, _ = O.rollout(envs, oa, 1, seed, id0, t, record=True)
        keys.append(k), acts.append(pi(g, a[0])), rews.append(r[0].astype(np.float32)), gs.append(g)
    keys, acts, rews, gs = (np.concatenate(x) for x in (keys, acts, rews, gs))
    visited = np.unique(canon(oa.dump()[0])[2])
    at = np.searchsorted(visited, keys)
    assert np.array_equal(visited[np.minimum(at, len(visited) - 1)], keys)       # every s has a row
    pair = at.astype(np.uint64) * np.uint64(4) + acts.astype(np.uint64)
    triples = np.unique((pair << np.uint64(32)) | value_bits(rews))
    return dict(boards=envs["board"][:, :16].copy(), visited=visited, pairs=np.unique(pair), triples=triples,
                turned=np.unique(pair[gs != 0]))


def value_bits(x):
    """float32 values as uint64 codes of their bit patterns, -0.0 as 0.0 (they compare equal)."""
    return (np.asarray(x, dtype=np.float32) + np.float32(0.0)).view(np.uint32).astype(np.uint64)


_ledgers = {}


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("strict", [False, True])
def test_shared_table_values(pkg, O, dev, strict):
    """lr = 1, gamma = 0: every write is Q[s][a] = reward, so whatever the interleaving a stored value is exactly one
    of the float32 rewards the oracle's games saw for (canonical key of s, pi_g(a)), an entry never taken is 0.0,
    and the rows are the canonical images of the states the oracle looked up.  A kernel that indexed the row with
    the env's action would put a reward under an action that never earned it.
    160 steps, not 64: one (state, action) earns several rewards mostly through the shaping state a reset keeps, and
    folding leaves an eighth of the plain pairs -- the oracle counts 264 such pairs after 64 steps (83 episodes
    over), 1179 after 128, 1490 after 160 (2896 episodes over); 528 076 rows, so 2^21 slots."""
    B, steps, seed, id0 = 4096, 160, 11, 500
    env = pkg.BatchedGame2048Env(B, 4, dev, seed, id0)
    agent = pkg.BatchedQLearningAgent(100, learning_rate=1.0, discount_factor=0.0, exploration_rate=1.0, capacity_log2=21,
                                      seed=seed, env_id0=id0, device=dev, placement="plain", strict_td=strict,
                                      freeze_load=None, symmetric=True)
    agent.fused_rollout(env, steps)
    sync(dev)
    if "ledger" not in _ledgers:
        _ledgers["ledger"] = shared_ledger(O, B, steps, seed, id0)
    L = _ledgers["ledger"]
    visited, pairs, triples = L["visited"], L["pairs"], L["triples"]
    assert np.array_equal(env.boards.cpu().numpy(), L["boards"]), "the oracle played other games"
    shared = int((np.unique(triples >> np.uint64(32), return_counts=True)[1] > 1).sum())
    print(f"strict {strict}: {len(visited)} rows, {len(pairs)} (key, action) pairs, {shared} with several rewards, "
          f"{len(L['turned'])} reached from a turned board")
    assert shared > 1000 and len(L["turned"]) > 1000                      # the race and the permutation are real
    dk, dq = agent.export_rows()
    order = np.argsort(dk)
    dk, dq = dk[order], dq[order]
    assert np.array_equal(dk, visited)                                   # every exported key is visited, and all are there
    assert np.array_equal(canon(unpack(dk))[2], dk)                      # ... and each is its own canonical image
    for act in range(4):
        pair = np.arange(len(dk), dtype=np.uint64) * np.uint64(4) + np.uint64(act)
        taken = np.isin(pair, pairs)
        legitimate = np.isin((pair << np.uint64(32)) | value_bits(dq[:, act]), triples)
        untouched = dq[:, act].view(np.uint32) == 0                      # exactly 0.0
        assert taken.any() and not taken.all() and np.where(taken, legitimate, untouched).all(), act
    st = agent.stats()
    assert len(dk) == len(visited) == st["inserts"] and st["drops"] == 0 and agent.check_status() == 0


# ---------------------------------------------------------------------------------------------
# 7. the folded player on every env profile
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("profile,rss", PROFILES)
def test_player_on_every_profile(pkg, O, dev, profile, rss):
    """The body of test_player_exploration_against_the_model: the rows the model decides on come from the numpy
    canonical form and a PLAIN lookup of the canonical boards, permuted here."""
    model_actions = importlib.import_module("test_play_rollout").model_actions
    B, steps, eps = 256, 120, 0.3
    with _quiet():
        env, agent = trained(pkg, dev, B, profile=profile, reset_shaping_state=rss)
    model = twin_of(pkg, env)
    _, reader = make(pkg, dev, B, False)
    reader.table = agent.table
    before = agent.table.clone()
    agent.play_rollout(env, 50, epsilon=eps)
    agent.play_rollout(env, steps - 50, epsilon=eps)
    explored = 0
    for _ in range(steps):
        cs, g, _ = canon(model.boards.cpu().numpy())
        q = env_rows(reader.q_values(t8(dev, cs)).cpu().numpy(), g)
        assert np.array_equal(q.view(np.uint32), bits(agent.q_values(model.boards)))
        acts, e = model_actions(O, q, model.legal_moves().cpu().numpy(), model.seed, model.env_id0, model.ctr, eps)
        explored += e
        _, _, done, _ = model.step(t8(dev, acts))
        model.reset(done)
    sync(dev)
    st = agent.play_stats()
    assert torch.equal(env.boards, model.boards) and torch.equal(env.aux, model.aux)
    assert st["explored"] == explored and 0.2 * B * steps < explored < 0.4 * B * steps
    assert st["steps"] == B * steps and st["episodes"] > 0 and torch.equal(agent.table, before)


# ---------------------------------------------------------------------------------------------
# 8. the 512-lane instantiations (batches of 786 432 boards and more): GPU only
# ---------------------------------------------------------------------------------------------
_big = {}


@pytest.mark.gpu
@pytest.mark.parametrize("strict", [False, True])
def test_big_batch(pkg, strict):
    """The first batch size that takes the 512-lane workgroups, with a tail block; epsilon 1, so a plain and a
    folded learner play the same games whatever their tables hold."""
    dev, B = "cuda:0", 786432 + 77
    env_p, plain = make(pkg, dev, B, False, cap=24, eps=1.0, strict_td=strict)
    env_s, folded = make(pkg, dev, B, True, cap=24, eps=1.0, strict_td=strict)
    plain.fused_rollout(env_p, 4)
    folded.fused_rollout(env_s, 4)
    sync(dev)
    assert torch.equal(env_p.boards, env_s.boards) and torch.equal(env_p.aux, env_s.aux)
    kp, _ = plain.export_rows()
    ks, _ = folded.export_rows()
    kp_sorted = np.sort(kp)
    if not ("plain" in _big and np.array_equal(_big["plain"], kp_sorted)):     # (both write modes play the same games)
        _big["plain"], _big["want"] = kp_sorted, np.unique(canon(unpack(kp))[2])
    want = _big["want"]
    assert np.array_equal(np.sort(ks), want)
    st = folded.stats()
    assert st["inserts"] == len(want) and st["drops"] == 0 and st["steps"] == 4 * B
    assert folded.check_status() == 0 and plain.check_status() == 0
    assert folded.verify_table()["rows"] == len(want) and plain.verify_table()["rows"] == len(kp)
    print(f"strict {strict}: rows plain {len(kp)} folded {len(ks)}")
    # evaluation, then the closed key set (with its line summaries): the same calls on both, no row more
    for agent, env in ((plain, env_p), (folded, env_s)):
        agent.fused_rollout(env, 4, learn=False)
        agent.frozen = True
        agent.fused_rollout(env, 4)
    sync(dev)
    assert torch.equal(env_p.boards, env_s.boards) and torch.equal(env_p.aux, env_s.aux)
    assert folded.table_size() == len(want) and plain.table_size() == len(kp)
    assert folded._summarised and folded.stats()["inserts"] == len(want) and folded.stats()["steps"] == 12 * B
    assert folded.check_status() == 0 and plain.check_status() == 0


# ---------------------------------------------------------------------------------------------
# 9. a tile above 2^15 is still reported
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_tile_overflow_is_still_reported(pkg, dev):
    """A 2^16 tile does not fit a key's nibble: the folded lookup and the folded rollout say so in the status word,
    as the plain ones do, return, and leave the other envs alone."""
    OVERFLOW = pkg._native.STATUS_TILE_OVERFLOW
    env_s, folded = make(pkg, dev, 64, True, cap=12, eps=1.0)
    env_p, plain = make(pkg, dev, 64, False, cap=12, eps=1.0)
    board = np.zeros(16, dtype=np.uint8)
    board[0], board[5] = 16, 1
    for env in (env_s, env_p):
        env.boards[7].copy_(t8(dev, board))
    assert folded.check_status() == 0
    folded.q_values(env_s.boards)
    assert folded.check_status() & OVERFLOW
    folded.status.zero_()
    others = torch.arange(64, device=dev) != 7
    folded.q_values(env_s.boards[others])
    assert folded.check_status() == 0                                    # (the other 63 boards do not set it)
    folded.fused_rollout(env_s, 1)
    plain.fused_rollout(env_p, 1)
    sync(dev)
    assert folded.check_status() & OVERFLOW and plain.check_status() & OVERFLOW
    assert torch.equal(env_s.boards[others], env_p.boards[others]) and torch.equal(env_s.aux[others], env_p.aux[others])
    assert int(env_s.boards[7].max()) == 16 and folded.stats()["steps"] == 64
