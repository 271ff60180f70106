"""Property tests: the CPU oracle == the reference, on random boards, actions, draws and shaping states.
The cases and the reference's answers to them are stored in golden G9 (tests/golden/g9_live_properties.npz,
written by `generate_golden.py --only-g9` with the reference imported live and driven by injected draws), so
these tests need only the oracle: thousands of cases per property, the input ranges of the reference's own
state space, one in ten draws taken from the edges of the u32 range."""
import numpy as np
import pytest

from conftest import load_npz


@pytest.fixture(scope="module")
def g9():
    return load_npz("g9_live_properties.npz")


def test_move_and_spawn(g9, O):
    n = len(g9["mv_board"])
    assert n >= 3000
    for i in range(n):
        board, action = g9["mv_board"][i].tolist(), int(g9["mv_action"][i])
        b, s, m = O.move(board, action)
        if m:
            b = O.add_number(b, int(g9["mv_dpos"][i]), int(g9["mv_dval"][i]))
        assert b.tolist() == g9["mv_want_board"][i].tolist(), i
        assert s == int(g9["mv_want_score"][i]) and m == bool(g9["mv_want_moved"][i]), i


def test_game_over_full_boards(g9, O):
    want = g9["go_want"]
    assert len(want) >= 3000 and 0 < int(want.sum()) < len(want)      # both answers occur
    for i, board in enumerate(g9["go_board"]):
        assert O.is_game_over(board.tolist()) == bool(want[i]), i


def test_env_step_reward_done_state(g9, O):
    n = len(g9["es_board"])
    assert n >= 3000
    for i in range(n):
        cons_count = int(g9["es_cons_count"][i])
        pen = -1.0
        for _ in range(max(0, cons_count - 10)):
            pen = max(pen * 1.1, -10)
        score0, prev, cons_action = int(g9["es_score0"][i]), int(g9["es_prev"][i]), int(g9["es_cons_action"][i])
        o = O.Env(4)
        o.set_board(g9["es_board"][i].tolist())
        rec = o.rec
        rec["score"][0], rec["previous_max_log2"][0] = score0, prev
        rec["consecutive_action"][0], rec["consecutive_count"][0] = cons_action, cons_count
        rec["last_consecutive_penalty"][0] = pen
        gb, gr, gd, gm, _ = o.step(int(g9["es_action"][i]), int(g9["es_dpos"][i]), int(g9["es_dval"][i]))
        got = (gb.tolist(), gr, gd, 1 << gm, int(rec["score"][0]), int(rec["previous_max_log2"][0]),
               int(rec["consecutive_count"][0]), float(rec["last_consecutive_penalty"][0]))
        want = (g9["es_want_board"][i].tolist(), float(g9["es_want_reward"][i]), bool(g9["es_want_done"][i]),
                int(g9["es_want_max"][i]), int(g9["es_want_score"][i]), int(g9["es_want_prev"][i]),
                int(g9["es_want_count"][i]), float(g9["es_want_penalty"][i]))
        assert got == want, i            # float64 reward and penalty bit-exact


def test_short_training_loops(g9, O):
    """120 steps of Agent/main.py:91-101 with injected draws == the oracle's rollout (dict too)."""
    loops = len(g9["tl_seed"])
    assert loops >= 60
    ends = np.cumsum(g9["tl_n_keys"])
    for i in range(loops):
        seed, env_id, eps = int(g9["tl_seed"][i]), int(g9["tl_env_id"][i]), float(g9["tl_eps"][i])
        keys, vals = g9["tl_q_keys"][ends[i] - g9["tl_n_keys"][i]:ends[i]], g9["tl_q_vals"][ends[i] - g9["tl_n_keys"][i]:ends[i]]
        envs = O.envs_init(1, 4, seed, env_id)
        agent = O.Agent(1000, 4, 0.1, 0.95, eps)
        si, sf, a, r, d = O.rollout(envs, agent, 120, seed, env_id, 0, record=True)
        assert np.array_equal(a[:, 0], g9["tl_actions"][i]) and np.array_equal(r[:, 0], g9["tl_rewards"][i]), i
        assert np.array_equal(d[:, 0], g9["tl_dones"][i]), i
        assert np.array_equal(envs["board"][:, :16], g9["tl_final_boards"][i:i + 1]) and len(agent) == len(keys), i
        assert np.array_equal(np.stack([agent.q(k) for k in keys]), vals), i


# ---- the DQN path's env (Deep_QLearning/environment/Game2048_nopenalty_env.py) ---------------------
def test_dqn_env_step(g9, O):
    """One step of the reference's second env (calculate_reward2, done = game_over, the board that
    is_game_over leaves in moved_board) == orc_env_step_dqn, both draw pairs routed as the build
    assigns them; boards weighted towards full ones (is_game_over's own moves only happen there)."""
    n = len(g9["dq_board"])
    assert n >= 3000
    for i in range(n):
        o = O.Env(4)
        o.set_board(g9["dq_board"][i].tolist())
        o.rec["score"][0] = int(g9["dq_score0"][i])
        d0, d1, d2, d3 = (int(x) for x in g9["dq_draws"][i])
        gb, gr, gd, gm, _ = o.step_dqn(int(g9["dq_action"][i]), d0, d1, d2, d3)
        want = (g9["dq_want_board"][i].tolist(), float(g9["dq_want_reward"][i]), bool(g9["dq_want_done"][i]),
                int(g9["dq_want_max"][i]), int(g9["dq_want_score"][i]))
        assert (gb.tolist(), gr, gd, (1 << gm) if gm else 0, int(o.rec["score"][0])) == want, i
