"""Every plain (not symmetry-folded) fused-learner variant against the float32 oracle.

On the device the fused rollout is one kernel per (board size N, env profile E, table mode, workgroup size), and the
deterministic step's first phase one per (N, E); on the CPU twin each is one function with run-time tests.  So every
case here runs on both.  The model everywhere is ONE oracle agent per env with float32 rows (`storage_f32=True`),
driven by `O.rollout` on that env alone with the device's launch cuts, `freeze()` where the device closes its key set;
the device agent has private rows (`independent=True`), so a lane is a function of its own id.  Boards, the integer aux
fields, every Q row (as float32 bit patterns) and the counters are compared EXACTLY; only the float32 running return
keeps the tolerance of test_no_learn_rollout_reads_but_never_writes.

Which case executes which instantiation (k_fused_rollout<N, E, mode, lanes>; N = 4 and 5 everywhere;
E = shaped, DQN, shaped + reset shaping, DQN + reset shaping = the four PROFILES):
  mode                      256 lanes, every (N, E)                     512 lanes, one E per mode (below)
  Learn                     test_learner_matrix[learn]                  test_big_batch[learn]
  Cas                       test_learner_matrix[cas]                    test_big_batch[cas]
  Eval                      test_evaluation_on_every_profile            test_big_batch[eval]
  Frozen                    test_learner_matrix[frozen]                 test_big_batch[frozen]
  Frozen+Cas                test_learner_matrix[frozen+cas]             test_big_batch[frozen+cas]
  Frozen+Summary            test_learner_matrix[frozen+summary]         test_big_batch[frozen+summary]
  Frozen+Summary+Cas        test_learner_matrix[frozen+summary+cas]     test_big_batch[frozen+summary+cas]
  play-only (E + play bit)  test_play_only_on_every_profile             test_big_batch[play], and the ageing launch
                                                                        of every test_big_batch case
  k_det_phase1<N, E>        test_deterministic_step_on_every_profile[open]   (N x E)
  k_det_phase1_visits<N, E> test_deterministic_step_on_every_profile[closed] (N x E)
  a second, ragged 256-lane workgroup (B = 333): test_learner_matrix, one profile per N, every mode
  512 lanes per workgroup   test_big_batch (GPU only): B = 786 432 + 77, one (E, mode) pair per mode --
                            (DQN, cas) (shaped + rs, eval) (DQN + rs, frozen) (shaped, frozen+cas) (DQN, frozen+summary)
                            (shaped + rs, frozen+summary+cas) (DQN + rs, learn) (DQN, play) -- plus the Learn kernel (Cas in
                            a compare-and-swap case) of each case's E in its 12 open steps and the play-only kernel of
                            its E in the ageing launch: 15 of the 32 instantiations per board size.
                            The other (E, mode) pairs at 512 lanes are left to the 256-lane matrix: the two differ in the
                            workgroup size alone.
Every 256-lane instantiation of the plain learner runs; of the 512-lane ones every mode and every profile, not every pair."""
import copy
import gc

import numpy as np
import pytest
import torch

from test_gpu_parity import oracle_aux
from test_symmetric_table import DEVICES, _quiet, sync

PROFILES = [("shaped", False), ("nopenalty", False), ("shaped", True), ("nopenalty", True)]
# table mode -> (strict_td, the key set closes, line_summaries)
MODES = {"learn": (False, False, True), "cas": (True, False, True), "frozen": (False, True, False),
         "frozen+cas": (True, True, False), "frozen+summary": (False, True, True),
         "frozen+summary+cas": (True, True, True)}
SEED, ID0, EPS, LR, GAMMA = 23, 7000, 0.3, 0.1, 0.95
FLOOR = 64                                  # episodes that must end in a case: the reset path ran
INT_STATS = ("steps", "episodes", "valid_moves", "score_sum", "explored")


def t8(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev)


def bits(a):
    """float32 values as their bit patterns."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle_flags(O, profile, rss):
    return (O.ENV_DQN if profile == "nopenalty" else 0) | (O.ENV_RESET_SHAPING if rss else 0)


def make(pkg, dev, n, B, profile, rss, cap, eps=EPS, strict=False):
    env = pkg.BatchedGame2048Env(B, n, dev, SEED, ID0, profile=profile, reset_shaping_state=rss)
    agent = pkg.BatchedQLearningAgent(100, learning_rate=LR, discount_factor=GAMMA, exploration_rate=eps,
                                      capacity_log2=cap, seed=SEED, env_id0=ID0, device=dev, independent=True,
                                      strict_td=strict, board_size=n, placement="plain", freeze_load=None)
    return env, agent


# ---------------------------------------------------------------------------------------------
# the model: one oracle agent per lane
# ---------------------------------------------------------------------------------------------
class Model:
    """Lanes `lanes` of a batch after `phases`, a list of (kind, steps, epsilon) that are the device's launches:
      "open"    the agent learns                        "closed"  the agent learns, its key set closed (`freeze()`)
      "eval"    the agent's learning rate is 0          "play"    a throw-away agent with learning rate 0: every row
                                                                  reads as zeros, nothing the learner holds is touched
    envs    the oracle's env records, one per lane      agents  the learners
    si      the oracle's integer statistics, summed over the lanes, one row per phase
    kept    per lane the learner's (keys, values) when the first "eval" or "play" phase began (else None)
    A model that tests share is not run further: `big_model` extends a copy."""

    def __init__(self, O, n, lanes, profile, rss):
        self.O, self.n, self.profile, self.rss = O, n, profile, rss
        self.lanes = np.asarray(lanes, dtype=np.int64)
        self.envs = np.concatenate([O.envs_init(1, n, SEED, ID0 + int(i)) for i in self.lanes])
        self.agents = [O.Agent(100, 4, LR, GAMMA, EPS, n=n, storage_f32=True) for _ in self.lanes]
        self.kept = [None] * len(self.lanes)
        self.si = np.zeros((0, O.ST_NI), dtype=np.int64)
        self.ctr = 0

    def run(self, phases):
        O, flags = self.O, oracle_flags(self.O, self.profile, self.rss)
        si = np.zeros((len(phases), O.ST_NI), dtype=np.int64)
        for j, lane in enumerate(self.lanes.tolist()):
            oa, ctr = self.agents[j], self.ctr
            for p, (kind, steps, eps) in enumerate(phases):
                if kind in ("eval", "play") and self.kept[j] is None:
                    self.kept[j] = oa.dump()
                if kind == "play":
                    who = O.Agent(100, 4, 0.0, GAMMA, eps, n=self.n, storage_f32=True)
                else:
                    who = oa
                    who.epsilon = eps
                    if kind == "closed":
                        who.freeze()
                    if kind == "eval":
                        who._view().lr = 0.0
                s, _ = O.rollout(self.envs[j:j + 1], who, steps, SEED, ID0 + lane, ctr, env_flags=flags)
                si[p] += s
                ctr += steps
        self.si = np.concatenate([self.si, si])
        self.ctr += sum(k for _, k, _ in phases)
        return self

    def total(self, first=0):
        return self.si[first:].sum(axis=0)

    def rows(self):
        return sum(len(oa) for oa in self.agents)

    def drops(self):
        return sum(oa.drops for oa in self.agents)

    def tables(self):
        """The learners' tables as one set of (lane, key bytes, four float32 bit patterns)."""
        out = set()
        for lane, oa in zip(self.lanes.tolist(), self.agents):
            keys, vals = oa.dump()
            out.update((lane, k.tobytes(), v.tobytes()) for k, v in zip(keys, bits(vals)))
        return out


def hist_of(O, si):
    return {1 << k: int(v) for k, v in enumerate(si[O.ST_HIST0:O.ST_HIST0 + 23]) if v}


def assert_lanes(dev, env, agent, m, kept=False):
    """The model's lanes on the device: boards, aux, and every row of every lane's learner as float32 bit patterns
    (`kept`: the rows as they were when the first evaluation or play-only launch began -- such a launch writes
    nothing, while the model's agent goes on creating zero rows)."""
    lanes = torch.from_numpy(m.lanes).to(dev)
    assert np.array_equal(env.boards[lanes].cpu().numpy(), m.envs["board"][:, :m.n * m.n]), "boards differ"
    aux = env.aux_fields()
    for k, v in oracle_aux(m.envs).items():
        assert np.array_equal(aux[k][m.lanes].astype(np.int64), np.asarray(v, dtype=np.int64)), k
    # the running return is a float32 sum on the device and a double in the oracle: not the subject here
    assert np.allclose(aux["ep_return"][m.lanes], m.envs["episode_return"], rtol=1e-4, atol=1e-3)
    rows = 0
    for j, lane in enumerate(m.lanes.tolist()):
        keys, vals = m.kept[j] if kept else m.agents[j].dump()
        rows += len(keys)
        if len(keys):
            got, found = agent.q_values(t8(dev, keys), env_id=ID0 + lane, return_found=True)
            assert bool(found.all()), lane
            assert np.array_equal(bits(got.cpu().numpy()), bits(vals)), lane
    return rows


def assert_counters(pkg, O, dev, agent, m, st, rows, drops):
    """The whole batch is the model's lanes: every counter is the oracle's sum."""
    si = m.total()
    for name, k in zip(INT_STATS, (O.ST_STEPS, O.ST_EPISODES, O.ST_VALID, O.ST_SCORE, O.ST_EXPLORE)):
        assert st[name] == int(si[k]), name
    assert st["max_tile_hist"] == hist_of(O, si)
    assert agent.table_size() == st["inserts"] == rows
    assert st["drops"] == drops
    assert agent.check_status() == 0
    assert pkg._native.claim_timeouts(pkg._native.lib_for(torch.device(dev))) == 0
    agent.verify_table()


# ---------------------------------------------------------------------------------------------
# 1. the learner matrix: board size x env profile x table mode, 256-lane workgroups
# ---------------------------------------------------------------------------------------------
OPEN1 = (1, 59)                                  # the key set open; then, open or closed as the mode has it:
REST1 = {4: (63, 177), 5: (63, 1377)}            # a visit row and the row cache cross a launch boundary (5x5 games are long)
RAGGED = {4: ("nopenalty", True), 5: ("shaped", True)}      # B = 333 as well: a second, ragged workgroup
_models, _learners = {}, {}


def batches(n):
    return [(n, p, r, B) for p, r in PROFILES for B in ((77, 333) if RAGGED[n] == (p, r) else (77,))]


CASES1 = batches(4) + batches(5)


def cap_for(rows):
    return max(8, int(np.ceil(np.log2(4.0 * rows))))    # load <= 0.25


def learner_model(O, n, profile, rss, B, closed):
    """One model for the modes that must agree: Learn and Cas (private rows: the compare-and-swap write equals the
    store), and the four closed ones (line summaries only shorten the lookup of an absent state)."""
    key = (n, profile, rss, B, closed)
    if key not in _models:
        kinds = ["open"] * len(OPEN1) + ["closed" if closed else "open"] * len(REST1[n])
        m = Model(O, n, range(B), profile, rss).run([(k, s, EPS) for k, s in zip(kinds, OPEN1 + REST1[n])])
        si = m.total()
        print(f"model {n}x{n} {profile} reset_shaping {rss} B {B} {'closed' if closed else 'open'}: episodes "
              f"{si[O.ST_EPISODES]} rows {m.rows()} drops {m.drops()} of {B * sum(REST1[n])} explored {si[O.ST_EXPLORE]} "
              f"of {si[O.ST_STEPS]}")
        _models[key] = m
    return _models[key]


def learner_run(pkg, O, dev, n, profile, rss, B, mode):
    """Each (device, n, profile, reset shaping, B, mode) runs once and is shared by the tests below."""
    key = (dev, n, profile, rss, B, mode)
    if key not in _learners:
        strict, closed, summaries = MODES[mode]
        steps = sum(OPEN1 + REST1[n])
        env, agent = make(pkg, dev, n, B, profile, rss, cap_for(B * steps), strict=strict)
        for k in OPEN1:
            agent.fused_rollout(env, k)
        if closed:
            agent.line_summaries = summaries
            agent.frozen = True                   # the key set is closed by hand (the policy has its own tests)
        for k in REST1[n]:
            agent.fused_rollout(env, k)
        sync(dev)
        _learners[key] = (env, agent)
    return _learners[key] + (learner_model(O, n, profile, rss, B, MODES[mode][1]),)


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n,profile,rss,B", CASES1)
def test_learner_matrix(pkg, O, dev, n, profile, rss, B, mode):
    """Launches of 1 and 59 steps with the key set open, then 63 and the rest in the case's mode: every lane is its
    oracle agent, and every counter the oracle's sum."""
    strict, closed, summaries = MODES[mode]
    env, agent, m = learner_run(pkg, O, dev, n, profile, rss, B, mode)
    st, si, steps = agent.stats(), m.total(), B * sum(OPEN1 + REST1[n])
    print(f"{n}x{n} {profile} reset_shaping {rss} B {B} {mode}: episodes {st['episodes']} rows {st['inserts']} "
          f"drops {st['drops']} explored {st['explored']} of {st['steps']}")
    rows = assert_lanes(dev, env, agent, m)
    assert rows == m.rows()
    assert_counters(pkg, O, dev, agent, m, st, rows, m.drops())
    # what keeps the case from passing vacuously; the model alone meets each of them
    assert st["steps"] == steps and si[O.ST_EPISODES] >= FLOOR, "the span must cover the reset path"
    assert 0.2 * steps < si[O.ST_EXPLORE] < 0.4 * steps, "both sides of the epsilon test"
    assert (m.drops() > 0.2 * B * sum(REST1[n])) if closed else m.drops() == 0, "the closed key set must bind"
    assert agent.frozen == closed and bool(agent.flags & pkg._native.FLAG_TD_CAS) == strict
    assert (agent._summarised if n == 4 else agent.side_summarised) == (closed and summaries)
    assert st["cas_retries"] == 0 and st["cas_fallbacks"] == 0, "private rows: no entry is shared"


@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("closed", [False, True])
def test_profiles_are_distinguishable_in_the_model(O, n, closed):
    """So that a kernel of the wrong profile cannot pass: what assert_lanes compares exactly differs between the
    profiles.  "shaped": reset shaping changes the aux records, and the tables while the key set is open (one that
    closed after 60 steps, before the first reset, holds almost only rows that no later game reaches: there the
    tables may agree).  "nopenalty" has no shaping state, so there reset shaping is inert by design (one model),
    and it differs from "shaped"."""
    def compared(m):
        return m.envs["board"].tobytes() + b"".join(np.asarray(v).tobytes() for v in oracle_aux(m.envs).values())

    plain, shaping = (learner_model(O, n, "shaped", r, 77, closed) for r in (False, True))
    dqn, dqn_shaping = (learner_model(O, n, "nopenalty", r, 77, closed) for r in (False, True))
    assert compared(plain) != compared(shaping) and (closed or plain.tables() != shaping.tables())
    assert dqn.envs.tobytes() == dqn_shaping.envs.tobytes() and dqn.tables() == dqn_shaping.tables()
    assert np.array_equal(dqn.si, dqn_shaping.si)
    assert compared(dqn) != compared(plain) and dqn.tables() != plain.tables()


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("n", [4, 5])
def test_reset_shaping_is_inert_without_shaping_state(pkg, O, dev, n, mode):
    """The two "nopenalty" kernels of a mode (with and without reset shaping) are one learner."""
    (env_a, a, _), (env_b, b, _) = (learner_run(pkg, O, dev, n, "nopenalty", r, 77, mode) for r in (False, True))
    assert torch.equal(env_a.boards, env_b.boards) and torch.equal(env_a.aux, env_b.aux)
    (ka, qa), (kb, qb) = a.export_rows(), b.export_rows()
    rows = [set(zip(map(bytes, np.ascontiguousarray(k).reshape(len(q), -1)), map(bytes, bits(q)))) for k, q in
            ((ka, qa), (kb, qb))]
    assert rows[0] == rows[1] and len(rows[0]) == len(qa) == len(qb) > 0


# ---------------------------------------------------------------------------------------------
# 2. evaluation and play-only on every profile
# ---------------------------------------------------------------------------------------------
EVAL2 = {4: (200, (37, 263)), 5: (300, (37, 1263))}          # training steps, the two evaluation launches
PLAY2 = {4: (63, 437), 5: (63, 1737)}
_evaluations, _players = {}, {}


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("profile,rss", PROFILES)
@pytest.mark.parametrize("n", [4, 5])
def test_evaluation_on_every_profile(pkg, O, dev, n, profile, rss):
    """`learn=False`: the table's bytes stay, nothing is created or dropped, and every trajectory is the oracle
    agent's that trained alongside and then had its learning rate set to 0."""
    B, (k1, cuts) = 77, EVAL2[n]
    key = (n, profile, rss)
    if key not in _evaluations:
        _evaluations[key] = Model(O, n, range(B), profile, rss).run([("open", k1, EPS)] + [("eval", k, EPS) for k in cuts])
    m = _evaluations[key]
    env, agent = make(pkg, dev, n, B, profile, rss, cap_for(B * k1))
    agent.fused_rollout(env, k1)
    before, st0, rows0 = agent.table.clone(), agent.stats(), agent.table_size()
    for k in cuts:
        agent.fused_rollout(env, k, learn=False)
    sync(dev)
    st, si = agent.stats(), m.total(1)
    print(f"{n}x{n} {profile} reset_shaping {rss} evaluation: episodes {si[O.ST_EPISODES]} explored {si[O.ST_EXPLORE]} "
          f"of {si[O.ST_STEPS]} rows {rows0}")
    assert torch.equal(agent.table, before), "an evaluation wrote to the table"
    assert st["inserts"] - st0["inserts"] == 0 and st["drops"] == 0 and agent.table_size() == rows0 == st["inserts"] > 0
    assert assert_lanes(dev, env, agent, m, kept=True) == rows0
    for name, k in zip(INT_STATS, (O.ST_STEPS, O.ST_EPISODES, O.ST_VALID, O.ST_SCORE, O.ST_EXPLORE)):
        assert st[name] - st0[name] == int(si[k]), name
    assert st["max_tile_hist"] == hist_of(O, m.total())
    assert agent.check_status() == 0
    agent.verify_table()
    assert si[O.ST_EPISODES] >= FLOOR and 0.2 * si[O.ST_STEPS] < si[O.ST_EXPLORE] < 0.4 * si[O.ST_STEPS]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("eps", [1.0, 0.3])
@pytest.mark.parametrize("profile,rss", PROFILES)
@pytest.mark.parametrize("n", [4, 5])
def test_play_only_on_every_profile(pkg, O, dev, n, profile, rss, eps):
    """No learner: every row reads as zeros (the greedy action is 0), the table -- far too small to learn in --
    stays all zeros."""
    B, cuts = 77, PLAY2[n]
    key = (n, profile, rss, eps)
    if key not in _players:
        _players[key] = Model(O, n, range(B), profile, rss).run([("play", k, eps) for k in cuts])
    m = _players[key]
    env, agent = make(pkg, dev, n, B, profile, rss, 6, eps=eps)
    for k in cuts:
        agent.fused_rollout(env, k, play_only=True)
    sync(dev)
    st, si, steps = agent.stats(), m.total(), B * sum(cuts)
    print(f"{n}x{n} {profile} reset_shaping {rss} play-only eps {eps}: episodes {si[O.ST_EPISODES]} explored "
          f"{si[O.ST_EXPLORE]} of {si[O.ST_STEPS]}")
    assert int(torch.count_nonzero(agent.table)) == 0
    assert assert_lanes(dev, env, agent, m, kept=True) == 0
    assert_counters(pkg, O, dev, agent, m, st, 0, 0)
    assert st["steps"] == steps and si[O.ST_EPISODES] >= FLOOR
    assert si[O.ST_EXPLORE] == steps if eps == 1.0 else 0.2 * steps < si[O.ST_EXPLORE] < 0.4 * steps


# ---------------------------------------------------------------------------------------------
# 3. the deterministic step on every profile
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("closed", [False, True], ids=["open", "closed"])
@pytest.mark.parametrize("profile,rss", PROFILES)
@pytest.mark.parametrize("n", [4, 5])
def test_deterministic_step_on_every_profile(pkg, O, dev, n, profile, rss, closed):
    """With private rows the two-phase semantic is the sequential one: the model is the learner matrix's."""
    B = 77
    m = learner_model(O, n, profile, rss, B, closed)
    env, agent = make(pkg, dev, n, B, profile, rss, cap_for(B * sum(OPEN1 + REST1[n])))
    for k in OPEN1:
        agent.deterministic_rollout(env, k)
    agent.frozen = closed
    for k in REST1[n]:
        agent.deterministic_rollout(env, k)
    sync(dev)
    st = agent.stats()
    print(f"{n}x{n} {profile} reset_shaping {rss} deterministic {'closed' if closed else 'open'}: episodes "
          f"{st['episodes']} rows {st['inserts']} drops {st['drops']} explored {st['explored']} of {st['steps']}")
    rows = assert_lanes(dev, env, agent, m)
    assert rows == m.rows()
    assert_counters(pkg, O, dev, agent, m, st, rows, m.drops())
    assert m.total()[O.ST_EPISODES] >= FLOOR and ((m.drops() > 0.2 * B * sum(REST1[n])) if closed else m.drops() == 0)


# ---------------------------------------------------------------------------------------------
# 4. the 512-lane instantiations (batches of 786 432 boards and more): GPU only
# ---------------------------------------------------------------------------------------------
BIG = 786432 + 77                    # the smallest batch size class of the 512-lane workgroups, with a ragged last one
AGE = {4: 90, 5: 600}                # steps of random play before the measured part: where first games end most often
LANES4 = {4: 500, 5: 1300}           # random lanes in the sample: enough to end FLOOR episodes in the 36 measured steps
OPEN4, REST4 = 12, (12, 12)
CASES4 = [("nopenalty", False, "cas"), ("shaped", True, "eval"), ("nopenalty", True, "frozen"),
          ("shaped", False, "frozen+cas"), ("nopenalty", False, "frozen+summary"),
          ("shaped", True, "frozen+summary+cas"), ("nopenalty", True, "learn"), ("nopenalty", False, "play")]
_aged = {}


def sampled_lanes(n_random):
    """Wave and workgroup edges of the first workgroups, the upper half of a middle workgroup, the last full
    workgroup's end, the first and the last lane of the ragged one, and random lanes."""
    fixed = [0, 63, 64, 255, 256, 511, 512, 512 * 700 + 300, 512 * 700 + 511, BIG - 78, BIG - 77, BIG - 1]
    rng = np.random.default_rng(5)
    return np.unique(np.concatenate([fixed, rng.integers(0, BIG, n_random)]))


def big_phases(mode):
    kind = mode if mode in ("eval", "play") else "closed" if MODES[mode][1] else "open"
    return [("open", OPEN4, EPS)] + [(kind, k, EPS) for k in REST4]


def big_model(O, n, profile, rss, mode):
    """The sampled lanes: aged by random play (a throw-away agent; once per env profile, then copied), then the
    measured launches."""
    key = (n, profile, rss)
    if key not in _aged:
        _aged[key] = Model(O, n, sampled_lanes(LANES4[n]), profile, rss).run([("play", AGE[n], 1.0)])
    aged = _aged[key]
    m = copy.copy(aged)                           # (the aged model keeps its envs; its learners are still untouched)
    m.envs, m.kept = aged.envs.copy(), [None] * len(aged.lanes)
    m.agents = [O.Agent(100, 4, LR, GAMMA, EPS, n=n, storage_f32=True) for _ in aged.lanes]
    return m.run(big_phases(mode))


@pytest.mark.gpu
@pytest.mark.parametrize("profile,rss,mode", CASES4)
@pytest.mark.parametrize("n", [4, 5])
def test_big_batch(pkg, O, n, profile, rss, mode):
    """Random play first (a fresh board ends no episode in a few dozen steps), then 12 steps with the key set open and
    twice 12 in the case's mode: the sampled lanes exactly as in the learner matrix, the whole batch by its counters."""
    big_case(pkg, O, "cuda:0", n, profile, rss, mode)
    gc.collect()
    torch.cuda.empty_cache()                      # each case's 2 GiB table goes back before the next


def big_case(pkg, O, dev, n, profile, rss, mode):
    steps = OPEN4 + sum(REST4)
    strict, closed, summaries = MODES.get(mode, (False, False, True))
    m = big_model(O, n, profile, rss, mode)
    env, agent = make(pkg, dev, n, BIG, profile, rss, 26, strict=strict)   # 2 GiB: load < 0.5 at one row per lane-step
    agent.epsilon = 1.0
    agent.fused_rollout(env, AGE[n], play_only=True)
    agent.epsilon = EPS
    aged = int(env.aux_fields()["episode"].astype(np.int64).sum())
    agent.stats(reset=True)
    agent.fused_rollout(env, OPEN4)
    st0, rows0 = agent.stats(), agent.table_size()
    if closed:
        agent.line_summaries = summaries
        agent.frozen = True
    with _quiet():
        for k in REST4:
            agent.fused_rollout(env, k, play_only=mode == "play", learn=mode != "eval")
    sync(dev)
    st, si = agent.stats(), m.total(1)
    print(f"{n}x{n} {profile} reset_shaping {rss} {mode} at {BIG} boards: {len(m.lanes)} sampled lanes end "
          f"{si[O.ST_EPISODES]} episodes, explore {si[O.ST_EXPLORE]} of {si[O.ST_STEPS]}, rows {m.rows()} drops "
          f"{m.drops()}; "
          f"the batch: episodes {st['episodes']} rows {st['inserts']} drops {st['drops']}")
    writes = mode not in ("eval", "play")
    assert_lanes(dev, env, agent, m, kept=not writes)
    assert si[O.ST_EPISODES] >= FLOOR, "the sampled lanes must cover the reset path"
    assert 0.2 * si[O.ST_STEPS] < si[O.ST_EXPLORE] < 0.4 * si[O.ST_STEPS]
    assert st["steps"] == BIG * steps
    assert st["episodes"] == int(env.aux_fields()["episode"].astype(np.int64).sum()) - aged
    if closed or not writes:
        assert st["inserts"] == st0["inserts"] == rows0 == agent.table_size()
    else:
        assert st["inserts"] == agent.table_size() > rows0
    assert (st["drops"] > 0.2 * BIG * sum(REST4) and m.drops() > 0) if closed else st["drops"] == 0
    assert (agent._summarised if n == 4 else agent.side_summarised) == (closed and summaries)
    assert st["cas_retries"] == 0 and agent.check_status() == 0
    assert pkg._native.claim_timeouts(pkg._native.lib_for(torch.device(dev))) == 0
    agent.verify_table()
