"""The row-tuple learner as a product: q2048_rt_play_rollout (the greedy player over the legal moves, on weights),
BatchedRowTupleAgent.play_rollout / play_stats / state_dict / load_state_dict, `train.py --agent row-tuple --save /
--resume / --eval-every`, `evaluate.py --model` on a row-tuple file, and merge_tables.py's refusal of one.

One launch plays `steps` steps of every env -- the row q2048_rt_lookup returns for the board, the legal-move mask, the
first maximum over the legal moves (or, exploring, the k-th legal move), the env step, statistics and the reset on
done -- and writes nothing but boards, aux and statistics.  So it is checked against code the package already has:
the four-call loop of `evaluate.play_legal_moves` at epsilon 0, a numpy model of the draw contract at epsilon > 0, and
(for the row itself) the numpy model of the row-tuple Q restated below.  Every comparison is exact: integers, bytes,
float32 bit patterns.  Every case runs on the CPU twin and on the GPU; the script cases run on the CPU twin with one
host thread (a learning run is then sequential and reproducible) and once on the GPU."""
import csv
import importlib
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
EDGES = [1, 63, 64, 65, 255, 256, 257, 1000]     # ends of a wave and of the 256-lane block, a ragged last wave
F32 = np.float32
SEED, ID0 = 11, 500
CUTS = (1, 63, 136)                              # 200 steps: a state carried wrongly across a launch shows
WARM = 100                                       # steps that take a fresh batch into mid-game before a comparison


# ---------------------------------------------------------------------------------------------
# the model of the row-tuple Q (plain numpy, no code shared with csrc/)
# ---------------------------------------------------------------------------------------------
def model_idx(boards, mask=15):
    """idx_r = sum_k (cell[4r+k] & 15) << 4k  -> int64 [B, 4]   (mask = 255: what a gather WITHOUT pack_row's mask reads)"""
    c = (np.asarray(boards, dtype=np.int64) & mask).reshape(-1, 4, 4)
    return c[:, :, 0] + (c[:, :, 1] << 4) + (c[:, :, 2] << 8) + (c[:, :, 3] << 12)


def model_q(W, boards, mask=15):
    """Q(s,a) = (W[0,idx_0,a] + W[1,idx_1,a]) + (W[2,idx_2,a] + W[3,idx_3,a]) in float32 -> float32 [B, 4]"""
    idx = model_idx(boards, mask)
    e0, e1, e2, e3 = (W[r, idx[:, r]] for r in range(4))
    assert e0.dtype == F32
    return (e0 + e1) + (e2 + e3)


def model_actions(O, q, legal, seed, id0, ctr, eps):
    """include/q2048.h, the player's draw contract: explore iff x0 < ceil(eps * 2^32) and a legal move exists; then the
    k-th legal move in ascending order, k = (x1 * n_legal) >> 32; else np.argmax of the masked row; no legal move: 0."""
    thr = 1 << 32 if eps >= 1.0 else 0 if eps <= 0.0 else math.ceil(eps * 4294967296.0)
    acts, explored = np.zeros(len(q), np.uint8), 0
    for i in range(len(q)):
        moves = [a for a in range(4) if (int(legal[i]) >> a) & 1]
        if not moves:
            continue
        x = O.draws(seed, id0 + i, ctr)
        if int(x[0]) < thr:
            acts[i] = moves[(int(x[1]) * len(moves)) >> 32]
            explored += 1
        else:
            acts[i] = int(np.argmax(np.where([(int(legal[i]) >> a) & 1 for a in range(4)], q[i], -np.inf)))
    return acts, explored


# ---------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------
def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def make_env(pkg, dev, B, profile="shaped", rss=False, seed=SEED, id0=ID0):
    return pkg.BatchedGame2048Env(B, 4, dev, seed, id0, profile=profile, reset_shaping_state=rss)


def make_agent(pkg, dev, eps=0.3, lr=0.1, seed=SEED, id0=ID0, epochs=100):
    return pkg.BatchedRowTupleAgent(epochs, learning_rate=lr, discount_factor=0.95, exploration_rate=eps, seed=seed,
                                    env_id0=id0, device=dev)


def twin_of(pkg, env):
    """A second env with the same boards, aux, seed and counter."""
    other = pkg.BatchedGame2048Env(env.num_envs, 4, env.device, env.seed, env.env_id0, profile=env.profile,
                                   reset_shaping_state=env.reset_shaping_state)
    other.load_state_dict(env.state_dict())
    return other


DEAD = torch.tensor([1 + ((r + c) & 1) for r in range(4) for c in range(4)], dtype=torch.uint8)   # full, no equal neighbours


def midgame(pkg, dev, B, profile="shaped", rss=False, dead=5):
    """An env batch WARM steps into its games -- aux records (scores, returns, action streaks, episode numbers) and step
    counter as a scratch learner left them (shaped steps: the learner takes no other), then given the asked profile --
    on CROWDED boards: 14 random tiles 2..128 and two empty cells, a few moves from the end of the game, so that every
    env ends an episode early in the span and plays a fresh game from its reset for the rest of it; `dead` dead boards
    planted in front."""
    scratch_env, scratch = make_env(pkg, dev, B), make_agent(pkg, dev)
    scratch.fused_rollout(scratch_env, WARM)
    env = make_env(pkg, dev, B, profile, rss)
    env.aux.copy_(scratch_env.aux)
    env.ctr = scratch_env.ctr
    rng = np.random.default_rng(B)
    boards = rng.integers(1, 8, (B, 16)).astype(np.uint8)
    for i in range(B):
        boards[i, rng.choice(16, 2, replace=False)] = 0
    k = min(dead, B)
    boards[:k] = DEAD.numpy()[None, :]
    env.boards.copy_(torch.from_numpy(boards).to(dev))
    return env, k


_WEIGHTS = {}


def weights_of(pkg, dev, kind):
    """The two weight sets of the comparison, made once per device and never written again:
    "trained": 300 steps of fused_rollout at 1000 boards;  "random": standard normal float32 over all of W."""
    if (dev, kind) not in _WEIGHTS:
        if kind == "trained":
            env, agent = make_env(pkg, dev, 1000), make_agent(pkg, dev)
            agent.fused_rollout(env, 300)
            sync(dev)
            w = agent.weights.clone()
        else:
            w = torch.from_numpy(np.random.default_rng(7).standard_normal((4, 65536, 4)).astype(F32)).to(dev)
        _WEIGHTS[(dev, kind)] = w
    return _WEIGHTS[(dev, kind)]


def agent_with(pkg, dev, kind, **kw):
    agent = make_agent(pkg, dev, **kw)
    agent.weights.copy_(weights_of(pkg, dev, kind))
    return agent


def four_call_loop(agent, env, steps):
    """`steps` steps of evaluate.play_legal_moves (epsilon 0) -- the loop the player replaces, itself: q2048_rt_lookup,
    q2048_legal_moves, env_step, env_reset."""
    evaluate = importlib.import_module("evaluate")
    args = types.SimpleNamespace(seed=env.seed, epsilon=0.0, steps_per_launch=int(steps), max_steps=env.ctr + int(steps))
    st = evaluate.play_legal_moves(torch, agent, env, args, 1 << 62)
    assert st["steps"] == steps * env.num_envs
    return st


# ---------------------------------------------------------------------------------------------
# 1. ABI: both libraries, argument errors, flags, no-ops, canaries
# ---------------------------------------------------------------------------------------------
def test_both_libraries_export_the_player(pkg):
    N = pkg._native
    assert "q2048_rt_play_rollout" in N._SIGNATURES
    assert hasattr(N.host_lib(), "q2048_rt_play_rollout") and N.host_lib().q2048_abi_version() == 7
    assert hasattr(N.lib(), "q2048_rt_play_rollout") and N.lib().q2048_abi_version() == 7 == N.ABI_VERSION
    with open(os.path.join(REPO, "include", "q2048.h")) as fh:
        assert "int q2048_rt_play_rollout(uint8_t *boards, q2048_aux *aux, const float *weights," in fh.read()


def argument_errors(f, b, a, w, s):
    """One call per argument error, in the order of the other entry points (B, flags, NULL, alignment, steps, eps);
    every call also carries the errors that come later in the order."""
    ok = lambda **kw: f(*[kw.get(k, d) for k, d in (("boards", b), ("aux", a), ("weights", w), ("B", 64), ("steps", 1),   # noqa: E731
                                                   ("eps", 0.0), ("seed", 1), ("id0", 0), ("ctr", 0), ("flags", 0),
                                                   ("si", None), ("sf", None), ("status", s), ("stream", None))])
    later = dict(B=-1, flags=64, weights=None, steps=-1, eps=2.0)
    assert ok(**later) == -2 and ok(**{**later, "B": (2 ** 31 - 1) * 256 + 1}) == -2   # SIZE: B
    del later["B"]
    assert ok(**later) == -7                                           # FLAGS
    del later["flags"]
    assert ok(**later) == -1                                           # NULL: weights
    del later["weights"]
    assert ok(boards=None, **later) == -1 and ok(aux=None, **later) == -1 and ok(status=None, **later) == -1
    assert ok(weights=w + 8, **later) == -3 and ok(boards=b + 8, **later) == -3 and ok(aux=a + 4, **later) == -3   # ALIGN
    assert ok(**later) == -2 and ok(**{**later, "steps": (1 << 30) + 1}) == -2   # SIZE: steps
    del later["steps"]
    assert ok(**later) == -6 and ok(eps=-0.5) == -6 and ok(eps=float("nan")) == -6   # RANGE
    return ok


@pytest.mark.parametrize("which", ["hip", "host"])
def test_argument_errors_need_no_device(pkg, which):
    """Both libraries check their arguments on the host before anything is launched or touched: made-up addresses do."""
    L = pkg._native.lib() if which == "hip" else pkg._native.host_lib()
    ok = argument_errors(L.q2048_rt_play_rollout, 0x1000, 0x2000, 0x3000, 0x4000)
    N = pkg._native
    for bit in (N.FLAG_INDEPENDENT, N.FLAG_SYMMETRIC, 1 << 30):
        assert ok(flags=bit) == -7 and ok(flags=bit | N.FLAG_ENV_DQN | N.FLAG_RESET_SHAPING) == -7, bit
    assert ok(B=0) == 0 and ok(steps=0) == 0                            # no-ops: nothing behind the addresses is touched
    assert ok(B=0, boards=None) == -1 and ok(steps=0, weights=0x3008) == -3 and ok(B=0, flags=N.FLAG_INDEPENDENT) == -7


@pytest.mark.parametrize("dev", DEVICES)
def test_refused_calls_write_nothing(pkg, dev):
    N = pkg._native
    L = N.lib_for(torch.device(dev))
    env, agent = make_env(pkg, dev, 64), agent_with(pkg, dev, "random")
    si, sf = pkg.agent.new_stats_vectors(torch.device(dev))
    env.aux.view(torch.uint8).fill_(0xA5)                              # canaries everywhere
    env.boards.fill_(0x5A)
    si.fill_(0x1234567)
    sf.fill_(-7.5)
    agent.status.fill_(0x777)
    before = [t.clone() for t in (env.boards, env.aux, si, sf, agent.status, agent.weights)]
    ok = argument_errors(L.q2048_rt_play_rollout, env.boards.data_ptr(), env.aux.data_ptr(), agent.weights.data_ptr(),
                         agent.status.data_ptr())
    stats = dict(si=si.data_ptr(), sf=sf.data_ptr())
    for bit in (N.FLAG_INDEPENDENT, N.FLAG_SYMMETRIC, N.FLAG_SINGLE_ENV, N.FLAG_TD_CAS, N.FLAG_PLAY_ONLY, N.FLAG_NO_LEARN,
                N.FLAG_NO_NEW_ROWS, N.FLAG_LINE_SUMMARY, 1 << 8, 1 << 23, 1 << 30, 1 << 31):
        assert ok(flags=bit, **stats) == -7 and ok(flags=bit | N.FLAG_ENV_DQN, **stats) == -7, bit
    assert ok(B=0, **stats) == 0 and ok(steps=0, **stats) == 0
    sync(dev)
    for got, want in zip((env.boards, env.aux, si, sf, agent.status, agent.weights), before):
        assert torch.equal(got, want)
    env2 = make_env(pkg, dev, 64)
    si.zero_()
    sf.zero_()
    ok2 = lambda **kw: ok(boards=env2.boards.data_ptr(), aux=env2.aux.data_ptr(), **kw)   # noqa: E731
    for flags in (0, N.FLAG_ENV_DQN, N.FLAG_RESET_SHAPING, N.FLAG_ENV_DQN | N.FLAG_RESET_SHAPING):
        assert ok2(flags=flags, steps=3, **stats) == 0
    assert ok2(steps=2) == 0                                            # statistics pointers may be NULL
    sync(dev)
    assert int(si[N.ST_STEPS]) == 4 * 3 * 64 and int(agent.status.item()) == 0x777   # status: required, never written
    assert torch.equal(bits(agent.weights), bits(before[5]))


# ---------------------------------------------------------------------------------------------
# 2. the main test: epsilon 0 == the four-call loop, byte for byte
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
@pytest.mark.parametrize("kind", ["trained", "random"])
@pytest.mark.parametrize("rss", [False, True])
@pytest.mark.parametrize("profile", ["shaped", "nopenalty"])
def test_equals_the_four_call_loop(pkg, dev, profile, rss, kind, B):
    """Mid-game state plus planted dead boards, then 200 steps played twice: by play_rollout in launches of 1 + 63 + 136
    and by evaluate.play_legal_moves on a second env with the same boards, seed and counter.  Boards, aux, every
    statistic and all 4 MiB of W (unchanged) are compared; at least one episode per env on average finishes.
    (Episodes per env inside the span, CPU twin: trained weights 1.09 .. 1.23 at B >= 63, random weights 2.1 .. 2.3.  On
    boards taken from running games the trained weights, whose games last about 250 steps, end only 0.72 .. 0.91
    episodes per env in 200 steps: hence the crowded boards of `midgame`; after its reset every env plays a real
    game for the rest of the span.)
    Random weights: every row differs, and the argmax over ALL four moves is an illegal move for a share of the lanes
    of the first step already (printed: 5 of 63 .. 20 of 1000 lanes on these boards -- the planted dead boards and the
    crowded boards on which a move changes nothing --, the planted board at B = 1; more follow as the games go on) --
    a player that ignored the mask would part from the loop there."""
    env, dead = midgame(pkg, dev, B, profile, rss)
    agent = agent_with(pkg, dev, kind)
    if kind == "random":
        W = weights_of(pkg, dev, kind).cpu().numpy()
        q = agent.q_values(env.boards).cpu().numpy()
        assert np.array_equal(q.view(np.uint32), model_q(W, env.boards.cpu().numpy()).view(np.uint32))   # the row's definition
        legal = env.legal_moves().cpu().numpy()
        illegal = int(((legal >> q.argmax(1)) & 1 == 0).sum())
        print(f"B {B}: the unmasked argmax is an illegal move for {illegal} lanes ({illegal / B:.3f})")
        assert illegal > 0
    env_loop = twin_of(pkg, env)
    w_before = bits(agent.weights).clone()
    train_stats = agent.stats_i.clone(), agent.stats_f.clone()
    for c in CUTS:
        agent.play_rollout(env, c)
    st_loop = four_call_loop(agent, env_loop, sum(CUTS))
    sync(dev)
    st = agent.play_stats()
    print(f"episodes fused {st['episodes']} loop {st_loop['episodes']} steps {st['steps']} valid {st['valid_moves']}")
    assert torch.equal(env.boards, env_loop.boards), "boards differ"
    assert torch.equal(env.aux, env_loop.aux), "aux records differ"
    assert env.ctr == env_loop.ctr == WARM + sum(CUTS)
    assert st["steps"] == st_loop["steps"] == B * sum(CUTS) and st["valid_moves"] == st_loop["valid_moves"]
    assert st["episodes"] == st_loop["episodes"] and st["max_tile_hist"] == st_loop["max_tile_hist"]
    assert st["score_sum"] == round(st_loop["mean_score"] * st_loop["episodes"])
    # float sums: only the order of a double sum differs (<= N * 2^-53 relative); 1e-9 * sqrt(sum x^2) <= 1e-9 * sum |x|
    assert abs(st["return_sum"] - st_loop["mean_return"] * st_loop["episodes"]) <= 1e-9 * math.sqrt(st["return_sq_sum"]) + 1e-300
    assert st["explored"] == 0 and st["inserts"] == 0 and st["drops"] == 0
    assert torch.equal(bits(agent.weights), w_before), "the player wrote to the weights"
    assert torch.equal(agent.stats_i, train_stats[0]) and torch.equal(agent.stats_f, train_stats[1])
    assert int(agent.status.item()) == 0
    assert st["episodes"] >= B and st["episodes"] >= dead, "the span must cover the reset path"


# ---------------------------------------------------------------------------------------------
# 3. epsilon > 0 against the model of the draw contract
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("eps", [0.3, 1.0])
def test_exploration_against_a_model(pkg, O, dev, eps):
    B, steps = 257, 40
    env, _ = midgame(pkg, dev, B, dead=3)
    agent = agent_with(pkg, dev, "random")
    model = twin_of(pkg, env)
    agent.play_rollout(env, 15, epsilon=eps)
    agent.play_rollout(env, steps - 15, epsilon=eps)
    explored = valid = 0
    for _ in range(steps):
        q = agent.q_values(model.boards).cpu().numpy()
        legal = model.legal_moves().cpu().numpy()
        acts, e = model_actions(O, q, legal, model.seed, model.env_id0, model.ctr, eps)
        explored += e
        valid += int((legal != 0).sum())                   # every move of the model is a legal one, where there is one
        _, _, done, _ = model.step(torch.from_numpy(acts).to(dev))
        model.reset(done)
    sync(dev)
    st = agent.play_stats()
    assert torch.equal(env.boards, model.boards) and torch.equal(env.aux, model.aux)   # the actions, through where they lead
    assert st["explored"] == explored and st["valid_moves"] == valid and st["steps"] == B * steps
    if eps == 1.0:
        assert explored == valid                           # every step with a legal move explores, no other
    else:
        assert 0.2 * B * steps < explored < 0.4 * B * steps


def one_move_board(action):
    """A board on which exactly `action` changes something: the line at the edge the tiles move to is empty, the rest is
    full without equal neighbours."""
    g = np.array([[1 + ((r + c) & 1) for c in range(4)] for r in range(4)], dtype=np.uint8)
    if action == 0: g[:, 0] = 0       # left: column 0 empty
    if action == 2: g[:, 3] = 0       # right
    if action == 1: g[0, :] = 0       # up: row 0 empty
    if action == 3: g[3, :] = 0       # down
    return g.reshape(-1)


@pytest.mark.parametrize("dev", DEVICES)
def test_epsilon_one_with_one_legal_move_or_none(pkg, dev):
    """epsilon = 1: a board with exactly one legal move takes it, for each of the four; a dead board takes action 0
    and is not counted as explored."""
    B = 260                                               # a partial wave, more than one block
    env, agent = make_env(pkg, dev, B), agent_with(pkg, dev, "random")
    want = np.arange(B) % 5                               # 4: the dead board
    boards = np.stack([one_move_board(a) if a < 4 else DEAD.numpy() for a in want])
    env.boards.copy_(torch.from_numpy(boards).to(dev))
    assert np.array_equal(env.legal_moves().cpu().numpy(), np.where(want < 4, 1 << want, 0))
    model = twin_of(pkg, env)
    agent.play_rollout(env, 1, epsilon=1.0)
    _, _, done, _ = model.step(torch.from_numpy(np.where(want < 4, want, 0).astype(np.uint8)).to(dev))
    model.reset(done)
    sync(dev)
    assert torch.equal(env.boards, model.boards) and torch.equal(env.aux, model.aux)
    st = agent.play_stats()
    assert st["explored"] == st["valid_moves"] == int((want < 4).sum()) and st["episodes"] == int(done.sum()) >= B // 5


# ---------------------------------------------------------------------------------------------
# 4. ties: all-zero weights take the first legal move;  5. a cell of 16 aliases to 0 in the player's gather
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_zero_weights_take_the_first_legal_move(pkg, dev):
    env, _ = midgame(pkg, dev, 333)
    agent = make_agent(pkg, dev)
    first = env.legal_moves().cpu().numpy()
    expect = np.array([0 if m == 0 else (int(m) & -int(m)).bit_length() - 1 for m in first], dtype=np.uint8)
    assert len(set(expect.tolist())) > 1                   # (not every lane's first legal move is action 0)
    model = twin_of(pkg, env)
    agent.play_rollout(env, 1)
    _, _, done, _ = model.step(torch.from_numpy(expect).to(dev))
    model.reset(done)
    sync(dev)
    assert torch.equal(env.boards, model.boards) and torch.equal(env.aux, model.aux)


@pytest.mark.parametrize("dev", DEVICES)
def test_a_cell_of_16_aliases_to_an_empty_one(pkg, dev):
    """Pairs of boards that differ only in cell 12: 0 against 16.  Rows 0 and 1 are 1 1 2 2 twice, so all four moves are
    legal on both boards whatever the rest holds, and the move is the plain argmax of the row -- the same row for both
    only if the player's gather takes the low nibble as pack_row does.  The move itself is read from the aux record
    (cons_action, the shaped env's last action), so nothing depends on what the step does with that cell.  A gather
    without the mask would read row table 3 one entry over (16 << 0 carries into the next nibble): by the model, that
    changes the move for a counted share of the pairs."""
    P = 200
    rng = np.random.default_rng(5)
    half = np.zeros((P, 16), np.uint8)
    half[:, 0:8] = [1, 1, 2, 2, 1, 1, 2, 2]
    half[:, 8:16] = rng.integers(1, 12, (P, 8))
    half[:, 12] = 0
    other = half.copy()
    other[:, 12] = 16
    env, agent = make_env(pkg, dev, 2 * P), agent_with(pkg, dev, "random")
    env.boards.copy_(torch.from_numpy(np.concatenate([half, other])).to(dev))
    assert (env.legal_moves().cpu().numpy() == 15).all()
    W = weights_of(pkg, dev, "random").cpu().numpy()
    want = model_q(W, half).argmax(1)
    unmasked = model_q(W, other, mask=255).argmax(1)
    print(f"a gather without the mask would move {int((unmasked != want).sum())} of {P} pairs differently")
    assert (unmasked != want).sum() > P // 4
    agent.play_rollout(env, 1)
    sync(dev)
    took = env.aux_fields()["cons_action"]
    assert np.array_equal(took[:P], want) and np.array_equal(took[P:], want)


# ---------------------------------------------------------------------------------------------
# 6. checkpoint
# ---------------------------------------------------------------------------------------------
def learner_state(agent, env):
    return (bits(agent.weights), env.boards.cpu(), env.aux.cpu(), agent.stats_i.cpu(), agent.stats_f.cpu(), agent.ctr,
            env.ctr, agent.epsilon)


def assert_same_state(a, b, weights=True):
    for k, (x, y) in enumerate(zip(a, b)):
        if k == 0 and not weights:
            continue
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y, k


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B,lr", [(1, 0.1), (1000, 0.0)])
def test_checkpoint_resumes_the_run(pkg, dev, B, lr):
    """120 steps, state_dict, a fresh agent and env, 80 more == 200 uninterrupted steps: at B = 1, where a learning run
    is a function of its inputs, in all of W (bit patterns), boards, aux, statistics, counters and epsilon; at B = 1000
    with lr = 0 (lanes race on W otherwise) in everything but W."""
    def run(cuts):
        env, agent = make_env(pkg, dev, B), make_agent(pkg, dev, eps=0.9, lr=lr, epochs=10)
        for k, steps in enumerate(cuts):
            agent.fused_rollout(env, steps)
            agent.decay_exploration(k)
            yield env, agent

    for env, agent in run([120, 80]):                      # uninterrupted: the same launches and decays, one agent
        pass
    whole = learner_state(agent, env)
    (env1, agent1), = run([120])
    sd, esd = agent1.state_dict(), env1.state_dict()
    assert sd["kind"] == "row_tuple" and sd["board_size"] == 4 and sd["weights"].device.type == "cpu"
    assert sd["weights"].dtype == torch.float32 and tuple(sd["weights"].shape) == (4, 65536, 4)
    assert set(sd) >= {"lr", "gamma", "schedule", "seed", "env_id0", "ctr", "stats_i", "stats_f"}
    env2, agent2 = make_env(pkg, dev, B, seed=1, id0=2), make_agent(pkg, dev, eps=0.1, lr=lr, seed=1, id0=2, epochs=10)
    agent2.load_state_dict(sd)
    env2.load_state_dict(esd)
    agent2.fused_rollout(env2, 80)
    agent2.decay_exploration(1)
    sync(dev)
    assert_same_state(learner_state(agent2, env2), whole, weights=(B == 1))
    assert agent2.stats()["episodes"] == agent.stats()["episodes"] and agent.stats()["steps"] == 200 * B


def test_checkpoints_of_the_two_kinds_do_not_cross_load(pkg):
    rt = make_agent(pkg, "cpu")
    ht = pkg.BatchedQLearningAgent(10, capacity_log2=12, device="cpu", placement="plain")
    with pytest.raises(ValueError, match="hash table"):
        rt.load_state_dict(ht.state_dict())
    with pytest.raises(ValueError, match="BatchedRowTupleAgent"):
        ht.load_state_dict(rt.state_dict())
    ht.load_state_dict(ht.state_dict())                    # (a dict without "kind" stays a hash table)


@pytest.mark.parametrize("dev", DEVICES)
def test_a_malformed_checkpoint_writes_nothing(pkg, dev):
    env, agent = make_env(pkg, dev, 64), make_agent(pkg, dev)
    agent.fused_rollout(env, 20)
    good = agent.state_dict()
    before = learner_state(agent, env)
    marked = dict(good, weights=good["weights"] + 1.0, ctr=999, stats_i=good["stats_i"] + 1)
    for bad in (dict(marked, weights=marked["weights"].double()), dict(marked, weights=marked["weights"][:, :4096]),
                dict(marked, weights=marked["weights"].numpy()), dict(marked, board_size=5),
                dict(marked, stats_i=marked["stats_i"].int()), dict(marked, stats_f=marked["stats_f"][:2]),
                {k: v for k, v in marked.items() if k != "kind"}):
        with pytest.raises(ValueError):
            agent.load_state_dict(bad)
        sync(dev)
        assert_same_state(learner_state(agent, env), before)
    agent.load_state_dict(marked)
    assert agent.ctr == 999 and torch.equal(agent.weights.cpu(), marked["weights"])


# ---------------------------------------------------------------------------------------------
# 7. the Python surface
# ---------------------------------------------------------------------------------------------
def test_python_surface(pkg):
    """`play_rollout` has the hash-table agent's semantics: the player is a function of (weights, env) -- seed, env_id0
    and the step counter are the ENV's, which is how `train.py --eval-every` plays a batch with a seed of its own
    while training goes on -- and it refuses what it cannot play: another device, a 5x5 env.  `fused_rollout` keeps
    its own checks (seed / env_id0 / ctr shared with the agent, no profile)."""
    env, agent = make_env(pkg, "cpu", 32), make_agent(pkg, "cpu")
    with pytest.raises(ValueError):
        agent.play_rollout(pkg.BatchedGame2048Env(32, 5, "cpu", SEED, ID0), 1)          # board size
    foreign = types.SimpleNamespace(device=torch.device("cuda:0"), board_size=4)
    with pytest.raises(ValueError, match="different devices"):
        agent.play_rollout(foreign, 1)
    assert agent.play_stats()["steps"] == 0
    agent.fused_rollout(env, 5)
    for kw in (dict(seed=SEED + 1), dict(id0=ID0 + 1)):
        with pytest.raises(ValueError):
            agent.fused_rollout(make_env(pkg, "cpu", 32, **kw), 1)                      # as before
    with pytest.raises(ValueError):
        agent.fused_rollout(make_env(pkg, "cpu", 32), 1)                                # (its counter is 0, the agent's 5)
    with pytest.raises(ValueError):
        agent.fused_rollout(make_env(pkg, "cpu", 32, profile="nopenalty"), 1)           # profiles: refused as before
    eval_env = make_env(pkg, "cpu", 48, profile="nopenalty", rss=True, seed=99, id0=12345)
    eval_env.ctr = 1000
    ctr, train_stats = agent.ctr, (agent.stats_i.clone(), agent.stats_f.clone())
    same = twin_of(pkg, eval_env)
    agent.play_rollout(eval_env, 7)
    four_call_loop(agent, same, 7)                         # ... on the env's own seed, ids, counter and profile
    assert torch.equal(eval_env.boards, same.boards) and torch.equal(eval_env.aux, same.aux)
    assert eval_env.ctr == 1007 and agent.ctr == ctr == 5
    assert torch.equal(agent.stats_i, train_stats[0]) and torch.equal(agent.stats_f, train_stats[1])   # never mixed
    st = agent.play_stats(reset=True)
    assert st["steps"] == 7 * 48 and set(st) == set(agent.stats()) and agent.stats()["steps"] == 5 * 32
    assert agent.play_stats()["steps"] == 0


# ---------------------------------------------------------------------------------------------
# 8. the scripts
# ---------------------------------------------------------------------------------------------
def script(tmp_path, device, name, *a):
    env = dict(os.environ, Q2048_HOST_THREADS="1")                      # the twin's rollout sequential: a learning run reproducible
    return subprocess.run([sys.executable, os.path.join(REPO, name), "--device", device, *a], capture_output=True,
                          text=True, timeout=600, cwd=str(tmp_path), env=env)


def load(tmp_path, name):
    return torch.load(tmp_path / name, map_location="cpu", weights_only=False)


def log_rows(tmp_path, name):
    return [r[:9] for r in list(csv.reader(open(tmp_path / name)))[1:]]   # (Steps/s, the wall clock's column, left out)


def test_train_save_resume_eval_and_the_other_scripts(pkg, tmp_path):
    train = ("train.py", "--agent", "row-tuple", "--num-envs", "64", "--episodes", "6", "--seed", "4",
             "--report-every", "1")
    run = lambda *a: script(tmp_path, "cpu", *train, *a)   # noqa: E731
    full = run("--save", "full.pt", "--log", "full.csv")
    assert full.returncode == 0, full.stderr[-2000:]
    part = run("--stop-epoch", "3", "--save", "part.pt", "--log", "p1.csv")
    assert part.returncode == 0, part.stderr[-2000:]
    rest = run("--resume", "part.pt", "--save", "resumed.pt", "--log", "p2.csv")
    assert rest.returncode == 0, rest.stderr[-2000:]
    a, b, p = (load(tmp_path, f) for f in ("full.pt", "resumed.pt", "part.pt"))
    assert a["kind"] == "row_tuple" and 3 <= p["train"]["epoch"] < 6 == a["train"]["epoch"] == b["train"]["epoch"]
    assert torch.equal(bits(a["weights"]), bits(b["weights"])) and bool(a["weights"].any())
    assert not torch.equal(bits(a["weights"]), bits(p["weights"]))
    assert a["ctr"] == b["ctr"] and torch.equal(a["stats_i"], b["stats_i"]) and torch.equal(a["stats_f"], b["stats_f"])
    assert a["schedule"] == b["schedule"]
    assert torch.equal(a["env"]["boards"], b["env"]["boards"]) and torch.equal(a["env"]["aux"], b["env"]["aux"])
    rows = log_rows(tmp_path, "full.csv")
    assert log_rows(tmp_path, "p1.csv") + log_rows(tmp_path, "p2.csv") == rows and rows[-1][0] == "6"
    # --eval-every: one JSON line per evaluation, the training log and the saved weights as without it
    ev = run("--save", "ev.pt", "--log", "ev.csv", "--eval-every", "2", "--eval-envs", "128", "--eval-log", "E.jsonl")
    assert ev.returncode == 0, ev.stderr[-2000:]
    e = load(tmp_path, "ev.pt")
    assert torch.equal(bits(a["weights"]), bits(e["weights"])) and log_rows(tmp_path, "ev.csv") == rows
    assert a["ctr"] == e["ctr"] and torch.equal(a["stats_i"], e["stats_i"]) and torch.equal(a["env"]["aux"], e["env"]["aux"])
    lines = [json.loads(ln) for ln in open(tmp_path / "E.jsonl").read().splitlines()]
    assert [ln["epoch"] for ln in lines] == [2, 4, 6]
    for ln in lines:
        assert ln["games"] >= 128 and sum(ln["max_tile_hist"].values()) == ln["games"] and 0.0 < ln["valid_move_frac"] <= 1.0
    # the refusals that stay
    for flag in (("--deterministic",), ("--episode-log", "ep.csv"), ("--symmetric",)):
        bad = run(*flag, "--log", "bad.csv")
        assert bad.returncode != 0 and flag[0] in bad.stderr, flag
    # evaluate.py: the same games with --fused and without; the reference policy leaves the weights alone too
    common = ("evaluate.py", "--model", "full.pt", "--num-envs", "96", "--episodes", "1", "--steps-per-launch", "32")
    plain, fused, ref = (script(tmp_path, "cpu", *common, *x) for x in ((), ("--fused",), ("--policy", "reference")))
    for r in (plain, fused, ref):
        assert r.returncode == 0, r.stderr[-2000:]
    x, y, z = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (plain, fused, ref))
    assert x["agent"] == y["agent"] == z["agent"] == "row-tuple" and y["fused"] is True and "rows" not in x
    assert set(y) == set(x) | {"fused"}
    for key in ("games", "env_steps", "mean_score", "max_tile_hist", "valid_move_frac"):
        assert x[key] == y[key], key
    assert x["games"] >= 96 and x["valid_move_frac"] > z["valid_move_frac"]
    # a hash-table file still evaluates as before, and says nothing of an agent
    h = script(tmp_path, "cpu", "train.py", "--num-envs", "64", "--steps-per-launch", "32", "--episodes", "2", "--max-steps",
               "64", "--capacity-log2", "14", "--save", "h.pt", "--log", "h.csv")
    assert h.returncode == 0, h.stderr[-2000:]
    hx = script(tmp_path, "cpu", "evaluate.py", "--model", "h.pt", "--num-envs", "64", "--fused")
    assert hx.returncode == 0 and "agent" not in json.loads(hx.stdout.strip().splitlines()[-1]), hx.stderr[-2000:]
    # cross-kind resume and merge are refused
    cross = run("--resume", "h.pt", "--log", "bad.csv")
    assert cross.returncode != 0 and "hash table" in cross.stderr
    merge = script(tmp_path, "cpu", "merge_tables.py", "full.pt", "resumed.pt", "--out", "m.pt")
    assert merge.returncode != 0 and "row-tuple weights" in merge.stderr and "not built" in merge.stderr
    assert not os.path.exists(tmp_path / "m.pt")


@pytest.mark.gpu
def test_evaluate_fused_on_weights_trained_on_the_device(pkg, tmp_path):
    t = script(tmp_path, "cuda", "train.py", "--agent", "row-tuple", "--num-envs", "1024", "--episodes", "3", "--save",
               "g.pt", "--log", "g.csv", "--eval-every", "1", "--eval-envs", "512", "--eval-log", "E.jsonl")
    assert t.returncode == 0, t.stderr[-2000:]
    assert [json.loads(ln)["epoch"] for ln in open(tmp_path / "E.jsonl").read().splitlines()] == [1, 2, 3]
    common = ("evaluate.py", "--model", "g.pt", "--num-envs", "1024", "--episodes", "1")
    plain, fused = script(tmp_path, "cuda", *common), script(tmp_path, "cuda", *common, "--fused")
    assert plain.returncode == 0 and fused.returncode == 0, plain.stderr[-2000:] + fused.stderr[-2000:]
    x, y = (json.loads(r.stdout.strip().splitlines()[-1]) for r in (plain, fused))
    assert y["agent"] == "row-tuple" and y["fused"] is True and y["games"] >= 1024
    for key in ("games", "env_steps", "mean_score", "max_tile_hist", "valid_move_frac"):
        assert x[key] == y[key], key
