"""The fused greedy player: q2048_play_rollout, BatchedQLearningAgent.play_rollout / play_stats,
`evaluate.py --fused`, `train.py --eval-every`.

One launch plays `steps` steps of every env -- the state's row, the legal-move mask, the first maximum over the
legal moves (or, exploring, the k-th legal move), the env step, statistics and reset on done -- and writes nothing
but boards, aux and statistics, so it is checked bit for bit against code the package already has: the four-call
loop of `evaluate.play_legal_moves` at epsilon 0, and a numpy model of the draw contract at epsilon > 0.  Every test
runs on the CPU twin and on the GPU."""
import ctypes as C
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

# Steps of the compared span (tests 2-4), chosen on the CPU twin so that the FOUR-CALL LOOP ALONE ends at least
# B / 4 episodes inside it for both board sizes, every profile and mode (the counts: docstring of test 2).
SPAN = {4: 160, 5: 160}


def sync(dev):
    if dev != "cpu":
        torch.cuda.synchronize()


def make(pkg, dev, B, n, profile="shaped", rss=False, independent=False, cap=16, seed=11, id0=500, eps=0.3, **kw):
    env = pkg.BatchedGame2048Env(B, n, dev, seed, id0, profile=profile, reset_shaping_state=rss)
    agent = pkg.BatchedQLearningAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=eps,
                                      capacity_log2=cap, seed=seed, env_id0=id0, device=dev, board_size=n,
                                      independent=independent, placement="plain", **kw)
    return env, agent


def twin_of(pkg, env):
    """A second env with the same boards, aux, seed and counter."""
    other = pkg.BatchedGame2048Env(env.num_envs, env.board_size, env.device, env.seed, env.env_id0,
                                   profile=env.profile, reset_shaping_state=env.reset_shaping_state)
    other.load_state_dict(env.state_dict())
    return other


def dead_board(n):
    """A full board without equal neighbours: no legal move."""
    return torch.tensor([1 + ((r + c) & 1) for r in range(n) for c in range(n)], dtype=torch.uint8)


def plant_dead(env, count):
    k = min(count, env.num_envs)
    env.boards[:k] = dead_board(env.board_size).to(env.device)[None, :]
    return k


def four_call_loop(pkg, agent, env, steps):
    """`steps` steps of evaluate.play_legal_moves (epsilon 0) -- the loop the player replaces, itself."""
    evaluate = importlib.import_module("evaluate")
    args = types.SimpleNamespace(seed=env.seed, epsilon=0.0, steps_per_launch=int(steps), max_steps=env.ctr + int(steps))
    st = evaluate.play_legal_moves(torch, agent, env, args, 1 << 62)
    assert st["steps"] == steps * env.num_envs
    return st


def play_in_launches(agent, env, steps, cuts=(1, 63)):
    left = steps
    for c in cuts:
        c = min(c, left)
        agent.play_rollout(env, c)
        left -= c
    agent.play_rollout(env, left)           # (0 steps left: a no-op)


def assert_same_games(dev, agent, env_fused, env_loop, st_loop, table_before, min_episodes):
    sync(dev)
    st = agent.play_stats()
    print(f"episodes fused {st['episodes']} loop {st_loop['episodes']} steps {st['steps']} valid {st['valid_moves']}")
    assert torch.equal(env_fused.boards, env_loop.boards), "boards differ"
    assert torch.equal(env_fused.aux, env_loop.aux), "aux records differ"
    assert env_fused.ctr == env_loop.ctr
    assert st["steps"] == st_loop["steps"] and st["valid_moves"] == st_loop["valid_moves"]
    assert st["episodes"] == st_loop["episodes"] and st["max_tile_hist"] == st_loop["max_tile_hist"]
    assert st["score_sum"] == round(st_loop["mean_score"] * st_loop["episodes"])
    # float sums: only the order of a double sum differs (<= N * 2^-53 relative); 1e-9 * sqrt(sum x^2) <= 1e-9 * sum |x|
    assert abs(st["return_sum"] - st_loop["mean_return"] * st_loop["episodes"]) <= 1e-9 * math.sqrt(st["return_sq_sum"]) + 1e-300
    assert st["explored"] == 0 and st["inserts"] == 0 and st["drops"] == 0
    assert torch.equal(agent.table, table_before), "the player wrote to the table"
    assert int(agent.status.item()) == 0
    assert st_loop["episodes"] >= min_episodes, "the span must cover the reset path"


# ---------------------------------------------------------------------------------------------
# 1. ABI
# ---------------------------------------------------------------------------------------------
def test_both_libraries_export_the_player(pkg):
    N = pkg._native
    assert "q2048_play_rollout" in N._SIGNATURES
    assert hasattr(N.host_lib(), "q2048_play_rollout") and N.host_lib().q2048_abi_version() == 7
    assert hasattr(N.lib(), "q2048_play_rollout") and N.lib().q2048_abi_version() == 7 == N.ABI_VERSION
    with open(os.path.join(REPO, "include", "q2048.h")) as fh:
        assert "int q2048_play_rollout(" in fh.read()


def argument_errors(f, b, a, t, s, cap=12, n=4):
    """One call per argument error, in the order of the other entry points; every call also carries the errors
    that come later in the order."""
    ok = lambda **kw: f(*[kw.get(k, d) for k, d in (("boards", b), ("aux", a), ("table", t), ("cap", cap), ("B", 64),   # noqa: E731
                                                   ("n", n), ("steps", 1), ("eps", 0.0), ("seed", 1), ("id0", 0),
                                                   ("ctr", 0), ("flags", 0), ("si", None), ("sf", None), ("status", s),
                                                   ("stream", None))])
    later = dict(B=-1, flags=64, table=None, boards=None, steps=-1, eps=2.0)
    assert ok(n=6, **later) == -4                                     # UNSUPPORTED
    assert ok(**later) == -2                                           # SIZE: B
    del later["B"]
    assert ok(**later) == -7                                           # FLAGS
    del later["flags"]
    assert ok(**later) == -1                                           # NULL: table
    del later["table"]
    assert ok(cap=3, **later) == -2 and ok(cap=41, **later) == -2      # SIZE: cap_log2
    assert ok(table=t + 8, **later) == -3                              # ALIGN: table
    assert ok(**later) == -1                                           # NULL: boards
    del later["boards"]
    assert ok(aux=None, **later) == -1 and ok(status=None, **later) == -1
    assert ok(boards=b + 8, **later) == -3 and ok(aux=a + 4, **later) == -3   # ALIGN
    assert ok(**later) == -2                                           # SIZE: steps
    del later["steps"]
    assert ok(**later) == -6 and ok(eps=-0.5) == -6 and ok(eps=float("nan")) == -6   # RANGE
    return ok


def test_argument_errors_of_the_hip_library_need_no_device(pkg):
    """The HIP library checks its arguments on the host before anything is launched: made-up addresses do."""
    argument_errors(pkg._native.lib().q2048_play_rollout, 0x1000, 0x2000, 0x3000, 0x4000)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_abi_errors_flags_and_noops(pkg, dev, n):
    N = pkg._native
    L = N.lib_for(torch.device(dev))
    env, agent = make(pkg, dev, 64, n, cap=12)
    si, sf = pkg.agent.new_stats_vectors(torch.device(dev))
    before = env.boards.clone(), env.aux.clone()
    ok = argument_errors(L.q2048_play_rollout, env.boards.data_ptr(), env.aux.data_ptr(), agent.table.data_ptr(),
                         agent.status.data_ptr(), cap=12, n=n)
    stats = dict(si=si.data_ptr(), sf=sf.data_ptr())
    refused = [N.FLAG_SINGLE_ENV, N.FLAG_TD_CAS, N.FLAG_PLAY_ONLY, N.FLAG_NO_LEARN, N.FLAG_NO_NEW_ROWS,
               N.FLAG_LINE_SUMMARY, N.FLAG_NO_NEW_ROWS | N.FLAG_LINE_SUMMARY, 1 << 8, 1 << 23, 1 << 30, 1 << 31]
    for bit in refused:
        assert ok(flags=bit, **stats) == -7, bit
        assert ok(flags=bit | N.FLAG_INDEPENDENT | N.FLAG_ENV_DQN, **stats) == -7, bit
    assert ok(B=0, **stats) == 0 and ok(steps=0, **stats) == 0          # no-ops
    assert ok(B=0, boards=None) == -1                                     # (arguments are still checked)
    sync(dev)
    assert torch.equal(env.boards, before[0]) and torch.equal(env.aux, before[1])
    assert not si.any() and not sf.any() and int(agent.status.item()) == 0
    for flags in (0, N.FLAG_INDEPENDENT, N.FLAG_ENV_DQN, N.FLAG_RESET_SHAPING,
                  N.FLAG_INDEPENDENT | N.FLAG_ENV_DQN | N.FLAG_RESET_SHAPING):
        assert ok(flags=flags, steps=3, **stats) == 0
    assert ok(steps=2) == 0                                               # statistics pointers may be NULL
    sync(dev)
    assert int(si[N.ST_STEPS]) == 5 * 3 * 64 and not torch.equal(env.boards, before[0])


def test_python_surface(pkg):
    env, agent = make(pkg, "cpu", 32, 4, cap=12)
    other = pkg.BatchedGame2048Env(32, 5, "cpu", 3, 7)
    with pytest.raises(ValueError):
        agent.play_rollout(other, 1)                                      # board size
    assert agent.play_stats()["steps"] == 0
    eval_env = pkg.BatchedGame2048Env(48, 4, "cpu", 99, 12345)          # another seed, id range, batch and counter
    eval_env.ctr = 1000
    agent.fused_rollout(env, 5)
    ctr, cache, train_stats = agent.ctr, agent._row_cache, (agent.stats_i.clone(), agent.stats_f.clone())
    agent.play_rollout(eval_env, 7)
    assert eval_env.ctr == 1007 and agent.ctr == ctr == 5 and agent._row_cache is cache
    assert torch.equal(agent.stats_i, train_stats[0]) and torch.equal(agent.stats_f, train_stats[1])   # never mixed
    st = agent.play_stats(reset=True)
    assert st["steps"] == 7 * 48 and set(st) == set(agent.stats())
    assert agent.play_stats()["steps"] == 0


# ---------------------------------------------------------------------------------------------
# 2. the main test: == the four-call loop at epsilon 0
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [1000, 77, 1])
@pytest.mark.parametrize("independent", [False, True])
@pytest.mark.parametrize("rss", [False, True])
@pytest.mark.parametrize("profile", ["shaped", "nopenalty"])
@pytest.mark.parametrize("n", [4, 5])
def test_equals_the_four_call_loop(pkg, dev, n, profile, rss, independent, B):
    """Mid-game boards and a table trained by `fused_rollout` (300 steps, capacity_log2 = 16: the key set closes on the
    way at B = 1000), five dead boards planted, then SPAN[n] steps played twice: by play_rollout in launches of 1, 63
    and the rest, and by evaluate.play_legal_moves on a second env with the same seed and counter.
    Episodes ended inside the 160-step span by the four-call loop alone (CPU twin; shared / independent rows):
      B = 1000 (needs 250)  4x4 shaped 925 / 884 (reset_shaping 935 / 884), nopenalty 871 / 918;
                            5x5 shaped 477 / 450, nopenalty 464 / 460 (the same with reset_shaping)
      B = 77 (needs 20)     4x4 66 .. 71, 5x5 33 .. 35;   B = 1: the planted board's game, 1 (needs 1)."""
    env, agent = make(pkg, dev, B, n, profile, rss, independent)
    with _quiet():
        for _ in range(5):
            agent.fused_rollout(env, 60)
    planted = plant_dead(env, 5)
    env_loop = twin_of(pkg, env)
    table_before = agent.table.clone()
    agent.status.zero_()
    play_in_launches(agent, env, SPAN[n])
    st_loop = four_call_loop(pkg, agent, env_loop, SPAN[n])
    assert_same_games(dev, agent, env, env_loop, st_loop, table_before, max(1, -(-B // 4)))
    assert st_loop["episodes"] >= planted


class _quiet:
    """The freeze warning of a table that fills up is expected here."""

    def __enter__(self):
        import warnings
        self._c = warnings.catch_warnings()
        self._c.__enter__()
        warnings.simplefilter("ignore")

    def __exit__(self, *exc):
        return self._c.__exit__(*exc)


# ---------------------------------------------------------------------------------------------
# 3. an untrained table: every state is absent, the action is the first legal move
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_empty_table(pkg, dev, n):
    B = 333
    env, agent = make(pkg, dev, B, n)
    agent.fused_rollout(env, 40, play_only=True)          # mid-game boards; the table stays empty
    assert agent.table_size() == 0
    plant_dead(env, 5)
    env_loop = twin_of(pkg, env)
    first = env.legal_moves().cpu().numpy()
    expect = np.array([0 if m == 0 else (int(m) & -int(m)).bit_length() - 1 for m in first])
    probe = twin_of(pkg, env)
    agent.play_rollout(probe, 1)
    stepped = twin_of(pkg, env)
    stepped.step(torch.from_numpy(expect.astype(np.uint8)).to(dev))
    stepped.reset(stepped._done)
    assert torch.equal(probe.boards, stepped.boards)      # the first legal move, env by env
    agent.play_stats(reset=True)
    table_before = agent.table.clone()
    play_in_launches(agent, env, SPAN[n])
    st_loop = four_call_loop(pkg, agent, env_loop, SPAN[n])
    assert_same_games(dev, agent, env, env_loop, st_loop, table_before, 5)


# ---------------------------------------------------------------------------------------------
# 4. a frozen 4x4 table with line summaries in its slots plays the same
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_frozen_table_with_line_summaries(pkg, dev):
    B = 256
    env, agent = make(pkg, dev, B, 4, cap=12, freeze_load=0.5)
    with _quiet():
        for _ in range(20):
            agent.fused_rollout(env, 16)
            if agent.frozen:
                break
        assert agent.frozen
        agent.fused_rollout(env, 16)                      # the first learning launch on the closed key set: summaries
    sync(dev)
    assert agent._summarised
    words = agent.table.view(torch.int64).reshape(-1, 4)
    assert bool((words[:, 3] != 0).any()), "no line summaries in the slots"
    plant_dead(env, 5)
    env_loop = twin_of(pkg, env)
    table_before = agent.table.clone()
    agent.status.zero_()
    play_in_launches(agent, env, SPAN[4])
    st_loop = four_call_loop(pkg, agent, env_loop, SPAN[4])
    assert_same_games(dev, agent, env, env_loop, st_loop, table_before, B // 4)


# ---------------------------------------------------------------------------------------------
# 5. epsilon > 0 against a model of the draw contract written here
# ---------------------------------------------------------------------------------------------
def model_actions(O, q, legal, seed, id0, ctr, eps):
    """include/q2048.h, q2048_play_rollout: explore iff x0 < ceil(eps * 2^32) and a legal move exists; then the k-th
    legal move in ascending order, k = (x1 * n_legal) >> 32; else np.argmax of the masked row; no legal move: 0."""
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


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_exploration_against_a_model(pkg, O, dev, n):
    B, steps, eps = 256, 150, 0.3
    env, agent = make(pkg, dev, B, n)
    agent.fused_rollout(env, 120)
    plant_dead(env, 3)
    model = twin_of(pkg, env)
    agent.play_rollout(env, 50, epsilon=eps)
    agent.play_rollout(env, steps - 50, epsilon=eps)
    explored = 0
    for _ in range(steps):
        q = agent.q_values(model.boards).cpu().numpy()
        legal = model.legal_moves().cpu().numpy()
        acts, e = model_actions(O, q, legal, model.seed, model.env_id0, model.ctr, eps)
        explored += e
        _, _, done, _ = model.step(torch.from_numpy(acts).to(dev))
        model.reset(done)
    sync(dev)
    st = agent.play_stats()
    assert torch.equal(env.boards, model.boards) and torch.equal(env.aux, model.aux)
    assert st["explored"] == explored and 0.2 * B * steps < explored < 0.4 * B * steps
    assert st["steps"] == B * steps and st["episodes"] > 0


def one_move_board(n, action):
    """A board on which exactly `action` changes something: the line at the edge the tiles move to is empty, the
    rest is full without equal neighbours."""
    g = np.array([[1 + ((r + c) & 1) for c in range(n)] for r in range(n)], dtype=np.uint8)
    if action == 0: g[:, 0] = 0       # left: column 0 empty
    if action == 2: g[:, n - 1] = 0   # right
    if action == 1: g[0, :] = 0       # up: row 0 empty
    if action == 3: g[n - 1, :] = 0   # down
    return g.reshape(-1)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("n", [4, 5])
def test_epsilon_one_with_a_single_legal_move(pkg, dev, n):
    B = 260                                               # a partial wave, more than one block
    env, agent = make(pkg, dev, B, n)
    agent.fused_rollout(env, 30)
    want = np.arange(B) % 4
    env.boards.copy_(torch.from_numpy(np.stack([one_move_board(n, a) for a in want])).to(dev))
    assert np.array_equal(env.legal_moves().cpu().numpy(), 1 << want)
    model = twin_of(pkg, env)
    agent.play_rollout(env, 1, epsilon=1.0)
    model.step(torch.from_numpy(want.astype(np.uint8)).to(dev))
    sync(dev)
    assert torch.equal(env.boards, model.boards) and torch.equal(env.aux, model.aux)
    st = agent.play_stats()
    assert st["explored"] == B == st["valid_moves"] and st["episodes"] == 0


# ---------------------------------------------------------------------------------------------
# 6. evaluate.py --fused
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_evaluate_fused_script(pkg, dev, tmp_path):
    device = "cpu" if dev == "cpu" else "cuda"
    py = lambda script, *a: subprocess.run([sys.executable, os.path.join(REPO, script), "--device", device, *a],   # noqa: E731
                                           capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    p = py("train.py", "--num-envs", "256", "--steps-per-launch", "32", "--episodes", "3", "--max-steps", "192",
           "--capacity-log2", "16", "--seed", "3", "--save", "q.pt", "--log", "log.csv")
    assert p.returncode == 0, p.stderr[-2000:]
    common = ("evaluate.py", "--model", "q.pt", "--num-envs", "192", "--episodes", "1", "--steps-per-launch", "32")
    plain, fused = py(*common), py(*common, "--fused")
    assert plain.returncode == 0, plain.stderr[-2000:]
    assert fused.returncode == 0, fused.stderr[-2000:]
    a, b = (json.loads(p.stdout.strip().splitlines()[-1]) for p in (plain, fused))
    assert "fused" not in a and b["fused"] is True and set(b) == set(a) | {"fused"}
    for key in ("games", "env_steps", "mean_score", "max_tile_hist", "valid_move_frac"):
        assert a[key] == b[key], key
    assert a["games"] >= 192
    bad = py(*common, "--fused", "--policy", "reference")
    assert bad.returncode != 0 and "--fused" in bad.stderr


# ---------------------------------------------------------------------------------------------
# 7. train.py --eval-every does not perturb training (CPU twin, deterministic mode)
# ---------------------------------------------------------------------------------------------
def test_eval_every_does_not_perturb_training(pkg, tmp_path):
    common = ["--device", "cpu", "--num-envs", "256", "--deterministic", "--episodes", "3", "--steps-per-launch", "32",
              "--report-every", "1", "--capacity-log2", "16", "--seed", "5"]
    run = lambda *a: subprocess.run([sys.executable, os.path.join(REPO, "train.py"), *common, *a],   # noqa: E731
                                    capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    p = run("--save", "a.pt", "--log", "a.csv")
    assert p.returncode == 0, p.stderr[-2000:]
    p = run("--save", "b.pt", "--log", "b.csv", "--eval-every", "1", "--eval-envs", "256", "--eval-log", "eval.jsonl")
    assert p.returncode == 0, p.stderr[-2000:]
    # the report rows, but for the wall-clock rate in the last column
    rows = [[line.rsplit(",", 1)[0] for line in open(tmp_path / f).read().splitlines()] for f in ("a.csv", "b.csv")]
    assert rows[0] == rows[1] and len(rows[0]) > 3
    a, b = (torch.load(tmp_path / f, map_location="cpu", weights_only=False) for f in ("a.pt", "b.pt"))
    for sd in (a, b):
        order = np.argsort(sd["keys"], kind="stable")
        sd["keys"], sd["q"] = sd["keys"][order], sd["q"][order]
    assert np.array_equal(a["keys"], b["keys"]) and np.array_equal(a["q"].view(np.uint32), b["q"].view(np.uint32))
    assert a["ctr"] == b["ctr"] and torch.equal(a["stats_i"], b["stats_i"]) and torch.equal(a["stats_f"], b["stats_f"])
    assert torch.equal(a["env"]["boards"], b["env"]["boards"]) and torch.equal(a["env"]["aux"], b["env"]["aux"])
    assert a["schedule"] == b["schedule"] and a["train"] == b["train"]
    lines = [json.loads(line) for line in open(tmp_path / "eval.jsonl").read().splitlines()]
    assert [e["epoch"] for e in lines] == list(range(1, a["train"]["epoch"] + 1)) and a["train"]["epoch"] == 3
    for e in lines:
        assert e["games"] >= 256 and set(e) >= {"epoch", "env_steps", "games", "mean_score", "mean_return",
                                                "max_tile_hist", "valid_move_frac"}
        assert sum(e["max_tile_hist"].values()) == e["games"] and 0.0 < e["valid_move_frac"] <= 1.0
    assert [e["env_steps"] for e in lines] == sorted(e["env_steps"] for e in lines)
