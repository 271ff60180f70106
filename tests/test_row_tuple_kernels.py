"""The row-tuple learner's entry points -- q2048_rt_choose, q2048_rt_lookup, q2048_rt_update, q2048_rt_fused_rollout --
against a numpy model, at batch sizes above one.

Which test executes which kernel (device) / function (CPU twin):
  k_rt_lookup         test_lookup_at_the_edges, test_lookup_and_greedy_choice_at_65536_boards
  k_rt_choose         test_choose_at_the_edges (greedy incl. exact ties; epsilon = 0.3 against the oracle's draws),
                      test_lookup_and_greedy_choice_at_65536_boards
  k_rt_update         test_update_on_rows_that_cannot_race (rt_gather of s and s', rt_delta, rt_scatter, the bad action)
  k_rt_fused_rollout  test_fused_rollout_with_frozen_weights (the carried entries, the gather after a reset, statistics),
                      test_fused_rollout_one_learning_step (rt_scatter inside the fused loop)
  the four argument checks   test_argument_checks

Tests 1-4 and 7 talk to the library through ctypes alone; the weights are a raw float32 [4, 65536, 4] tensor, so the
entry point under test is the only product code between the model and the assertion.  Tests 5 and 6 drive
BatchedRowTupleAgent / BatchedGame2048Env against the sequential oracle, on inputs where the sequential learner IS the
specification at any batch size (frozen weights; one step on rows no two lanes share).

The model (model_idx, model_q, model_update) is plain numpy and shares no code with csrc/.  Every comparison is exact:
integers, and float32 values as uint32 bit patterns.  There is no tolerance: Q is a fixed chain of float32 additions,
the TD step one float64 expression rounded once, and a contraction of reward + (gamma * max) * mask into an fma cannot
change it because the mask is 0.0 or 1.0.  Every test runs on the CPU twin ("cpu") and on the GPU."""
import numpy as np
import pytest
import torch

from test_gpu_parity import assert_aux

DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
EDGES = [1, 63, 64, 65, 255, 256, 257, 1000]     # ends of a wave and of a 256-lane block, a partial second block, four blocks
ROOM = 64                                        # canaried records beyond B in every output buffer
Q_CANARY, A_CANARY = 0xDEADBEEF, 0xA5
BAD_ACTION = 1                                   # Q2048_STATUS_BAD_ACTION
ERR_NULL, ERR_SIZE, ERR_ALIGN, ERR_RANGE = -1, -2, -3, -6
GRID_LIMIT = (2 ** 31 - 1) * 256                 # one block per 256 lanes, at most 2^31 - 1 blocks
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def model_idx(boards):
    """idx_r = sum_k (cell[4r+k] & 15) << 4k  -> int64 [B, 4]"""
    c = (np.asarray(boards, dtype=np.int64) & 15).reshape(-1, 4, 4)
    return c[:, :, 0] | (c[:, :, 1] << 4) | (c[:, :, 2] << 8) | (c[:, :, 3] << 12)


def model_q(W, boards):
    """Q(s,a) = (W[0,idx_0,a] + W[1,idx_1,a]) + (W[2,idx_2,a] + W[3,idx_3,a]) in float32 -> float32 [B, 4]"""
    idx = model_idx(boards)
    e0, e1, e2, e3 = (W[r, idx[:, r]] for r in range(4))
    assert e0.dtype == F32
    return (e0 + e1) + (e2 + e3)


def model_update(W, s, actions, reward, s2, done, lr, gamma):
    """The TD step, lane after lane on one array.  -> (weights afterwards, status word)"""
    W, status = W.copy(), 0
    idx_s = model_idx(s)
    for i in range(len(s)):
        a = int(actions[i])
        if a > 3:
            status |= BAD_ACTION
            continue
        max_next = float(model_q(W, s2[i:i + 1])[0].max())
        q_sa = float(model_q(W, s[i:i + 1])[0, a])
        target = float(reward[i]) + gamma * max_next * (0.0 if done[i] else 1.0)     # float64
        d = F32((lr * 0.25) * (target - q_sa))                                       # rounded once
        for r in range(4):
            W[r, idx_s[i, r], a] = F32(W[r, idx_s[i, r], a] + d)
    return W, status


def boards_of(idx):
    """int [B, 4] row indices -> uint8 [B, 16] boards (the inverse of model_idx on cells 0..15)"""
    idx = np.asarray(idx, dtype=np.int64)
    return np.stack([(idx[:, r] >> (4 * k)) & 15 for r in range(4) for k in range(4)], axis=1).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# the entry points, through ctypes alone
# ---------------------------------------------------------------------------------------------------------------
def lib(pkg, dev):
    return pkg._native.lib_for(torch.device(dev))


def t8(dev, a):
    """A tensor of its own on `dev` (on "cpu" too: never a view of the numpy array)."""
    return torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).to(dev)


def t32(dev, a):
    return torch.from_numpy(np.array(a, dtype=F32, order="C")).to(dev)


def bits(a):
    """float32 values as their bit patterns (numpy uint32)."""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a, dtype=F32)
    return a.view(np.uint32)


def assert_same_bits(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    bad = got != want
    assert not bad.any(), f"{what}: {int(bad.sum())} values differ, first at {np.argwhere(bad)[0].tolist()}"


def rt_lookup(L, dev, weights, boards):
    """q2048_rt_lookup into a canaried buffer -> (bit patterns uint32 [B, 4], the ROOM records behind them)"""
    B = len(boards)
    out = torch.full((B + ROOM, 4), Q_CANARY - (1 << 32), dtype=torch.int32, device=dev)
    tb = t8(dev, boards)
    assert L.q2048_rt_lookup(weights.data_ptr(), tb.data_ptr(), B, out.data_ptr(), None) == 0
    out = out.cpu().numpy().view(np.uint32)
    return out[:B], out[B:]


def rt_choose(L, dev, weights, boards, eps, seed=0, env_id0=0, ctr=0):
    """q2048_rt_choose into a canaried buffer -> (actions uint8 [B], the ROOM bytes behind them)"""
    B = len(boards)
    out = torch.full((B + ROOM,), A_CANARY, dtype=torch.uint8, device=dev)
    tb = t8(dev, boards)
    assert L.q2048_rt_choose(weights.data_ptr(), tb.data_ptr(), B, float(eps), seed, env_id0, ctr, out.data_ptr(),
                             None) == 0
    out = out.cpu().numpy()
    return out[:B], out[B:]


_SHARED = {}


def base_weights():
    """Random normal float32 [4, 65536, 4], built once; nobody writes it."""
    if "w" not in _SHARED:
        w = np.random.default_rng(20).standard_normal((4, 65536, 4)).astype(F32)
        w.setflags(write=False)
        _SHARED["w"] = w
    return _SHARED["w"]


def random_boards(rng, B):
    return rng.integers(0, 16, size=(B, 16), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# 1. rt_lookup at the edges
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
def test_lookup_at_the_edges(pkg, dev, B):
    """Random weights, random cells 0..15; lane 0 carries one cell of 16, which pack_row's mask reads as cell 0 (the
    model: & 15).  The 64 records beyond B keep their canary; the weights are not written."""
    L, W = lib(pkg, dev), base_weights()
    boards = random_boards(np.random.default_rng(100 + B), B)
    boards[0, 5] = 16
    as_zero = boards[:1].copy()
    as_zero[0, 5] = 0
    want = model_q(W, boards)
    assert_same_bits(want[:1], model_q(W, as_zero), "the model's own mask")
    boards[0, 5] = 3
    assert (bits(model_q(W, boards[:1])) != bits(want[:1])).any(), "cell 5 of lane 0 does not show in its row"
    boards[0, 5] = 16
    weights = t32(dev, W)
    got, tail = rt_lookup(L, dev, weights, boards)
    assert_same_bits(got.view(F32), want, f"B = {B}")
    assert (tail == np.uint32(Q_CANARY)).all(), "rows written beyond B"
    assert_same_bits(weights, W, "a lookup wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 2. rt_choose at the edges
# ---------------------------------------------------------------------------------------------------------------
TIES = [(0.5, 1.5, 1.5, -1.0), (0.25, -1.0, 2.0, 2.0), (-1.0, 3.0, 0.0, 3.0), (0.0, 0.0, 0.0, 0.0)]   # -> 1, 2, 1, 0


def weights_with_ties(B, boards):
    """base_weights() with hand-set entries: lane 0's four entries all zero (a zero row: action 0), and on up to five
    more lanes the entries of rows 1..3 zero and the entry of row 0 a row of TIES, whose maximum two actions share.
    -> (weights, the tied lanes, the action each must get)"""
    W = base_weights().copy()
    idx = model_idx(boards)
    lanes = [0] + sorted({i for i in (1, 62, 63, 64, B - 1) if 0 < i < B})
    rows = [TIES[3]] + [TIES[k % 3] for k in range(len(lanes) - 1)]
    for lane, row in zip(lanes, rows):
        for r in range(4):
            W[r, idx[lane, r]] = 0.0
    for lane, row in zip(lanes, rows):
        W[0, idx[lane, 0]] = row
    first = [int(np.argmax(np.asarray(row, dtype=F32))) for row in rows]
    # two special lanes could share an entry (random boards): what the lanes read is checked, not assumed
    q = model_q(W, boards[lanes])
    for k, row in enumerate(rows):
        assert np.array_equal(q[k], np.asarray(row, dtype=F32)), f"lane {lanes[k]} does not read its hand-set row"
    return W, lanes, first


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
def test_choose_at_the_edges(pkg, O, dev, B):
    """epsilon = 0: the model's argmax (the first maximum wins), on lanes with an exact tie too.  epsilon = 0.3 with
    (seed, env_id0, ctr) = (7, 2^33 + 5, 3): lane i explores when draw_uniform(x0) < epsilon and then takes
    draw_action(x1), x = the oracle's draws of env env_id0 + i.  Both branches occur and some greedy lane takes another
    action than zero weights would give -- asserted for B >= 63: one lane takes one branch, and with 63 lanes a branch
    stays empty with probability 0.7^63 < 2e-10."""
    L = lib(pkg, dev)
    boards = random_boards(np.random.default_rng(200 + B), B)
    W, lanes, first = weights_with_ties(B, boards)
    weights = t32(dev, W)
    greedy = np.argmax(model_q(W, boards), axis=1).astype(np.uint8)
    assert greedy[lanes].tolist() == first
    if B > 1:
        assert any(a > 0 for a in first), "no tie between two non-first actions"
    got, tail = rt_choose(L, dev, weights, boards, 0.0)
    assert np.array_equal(got, greedy), f"greedy actions differ on lanes {np.flatnonzero(got != greedy)[:8].tolist()}"
    assert (tail == A_CANARY).all(), "actions written beyond B"

    eps, seed, id0, ctr = 0.3, 7, (1 << 33) + 5, 3
    x = np.stack([O.draws(seed, id0 + i, ctr) for i in range(B)])
    explore = np.array([O.draw_uniform(v) < eps for v in x[:, 0]])
    want = np.where(explore, [O.draw_action(v) for v in x[:, 1]], greedy).astype(np.uint8)
    if B >= 63:
        assert explore.any() and not explore.all()
        assert (want[~explore] != 0).any(), "every greedy lane takes what zero weights would give"
    got, tail = rt_choose(L, dev, weights, boards, eps, seed, id0, ctr)
    assert np.array_equal(got, want), f"actions differ on lanes {np.flatnonzero(got != want)[:8].tolist()}"
    assert (tail == A_CANARY).all(), "actions written beyond B"
    assert_same_bits(weights, W, "choosing wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 3. rt_update on rows that cannot race
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", EDGES)
def test_update_on_rows_that_cannot_race(pkg, dev, B):
    """Per row position the B row indices of s are distinct and below 0x8000 (a slice of a permutation of 32768), and
    every row index of s' is at or above 0x8000: no lane reads an entry another lane writes, the result does not depend
    on the order of the lanes, and the sequential model is the specification.  The whole 4 MiB of weights is compared,
    so nothing but the 4 entries of each good lane moved.  One lane carries action 7 (B > 2): it writes nothing and
    sets Q2048_STATUS_BAD_ACTION."""
    L, W = lib(pkg, dev), base_weights()
    rng = np.random.default_rng(300 + B)
    s = boards_of(np.stack([rng.permutation(32768)[:B] for _ in range(4)], axis=1))
    s2 = boards_of(rng.integers(0x8000, 0x10000, size=(B, 4)))
    idx = model_idx(s)
    assert all(len(np.unique(idx[:, r])) == B for r in range(4)) and idx.max() < 0x8000 and model_idx(s2).min() >= 0x8000
    actions = rng.integers(0, 4, size=B, dtype=np.uint8)
    bad = B // 2 if B > 2 else None
    if bad is not None:
        actions[bad] = 7
    reward = rng.standard_normal(B).astype(F32)
    done = (rng.random(B) < 0.3).astype(np.uint8)
    lr, gamma = 0.1, 0.97
    want, want_status = model_update(W, s, actions, reward, s2, done, lr, gamma)
    good = B - (bad is not None)
    assert want_status == (BAD_ACTION if bad is not None else 0)
    assert int((bits(want) != bits(W)).sum()) == 4 * good          # every good lane moves its four entries

    weights, status = t32(dev, W), torch.zeros(1, dtype=torch.int32, device=dev)
    ts, ts2, ta, tr, td = t8(dev, s), t8(dev, s2), t8(dev, actions), t32(dev, reward), t8(dev, done)
    assert L.q2048_rt_update(weights.data_ptr(), ts.data_ptr(), ta.data_ptr(), tr.data_ptr(), ts2.data_ptr(),
                             td.data_ptr(), B, lr, gamma, status.data_ptr(), None) == 0
    got = weights.cpu().numpy()
    assert int(status.item()) == want_status
    assert_same_bits(got, want, f"B = {B}")
    assert int((bits(got) != bits(W)).sum()) == 4 * good
    for t, a in ((ts, s), (ts2, s2), (ta, actions), (td, done)):
        assert np.array_equal(t.cpu().numpy(), a), "an input was written"
    assert_same_bits(tr, reward, "the rewards were written")


# ---------------------------------------------------------------------------------------------------------------
# 4. the quoted batch size
# ---------------------------------------------------------------------------------------------------------------
def midgame_boards(O):
    """65,536 boards after 40 uniformly random steps of the oracle's envs, with the model's rows on base_weights()."""
    if "mid" not in _SHARED:
        B = 65536
        envs = O.envs_init(B, 4, 41, 0)
        O.rollout(envs, None, 40, 41, 0, 0)
        boards = envs["board"][:, :16].copy()
        assert boards.max() >= 5 and len(np.unique(boards, axis=0)) > B // 2
        q = model_q(base_weights(), boards)
        for a in (boards, q):
            a.setflags(write=False)
        _SHARED["mid"] = (boards, q)
    return _SHARED["mid"]


@pytest.mark.parametrize("dev", DEVICES)
def test_lookup_and_greedy_choice_at_65536_boards(pkg, O, dev):
    """The batch size the README's figure is quoted at: 256 full blocks, mid-game boards (hot row entries shared by
    most of the batch, as in a rollout).  Rows bit for bit, greedy actions equal; the model is vectorised numpy."""
    L, W = lib(pkg, dev), base_weights()
    boards, want = midgame_boards(O)
    weights = t32(dev, W)
    got, tail = rt_lookup(L, dev, weights, boards)
    assert_same_bits(got.view(F32), want, "65,536 boards")
    assert (tail == np.uint32(Q_CANARY)).all(), "rows written beyond B"
    greedy = np.argmax(want, axis=1).astype(np.uint8)
    assert np.bincount(greedy, minlength=4).min() > 0
    got, tail = rt_choose(L, dev, weights, boards, 0.0, 41, 0, 40)
    assert np.array_equal(got, greedy), f"{int((got != greedy).sum())} greedy actions differ"
    assert (tail == A_CANARY).all(), "actions written beyond B"
    assert_same_bits(weights, W, "a read-only pass wrote the weights")


# ---------------------------------------------------------------------------------------------------------------
# 5. fused rollout with frozen weights
# ---------------------------------------------------------------------------------------------------------------
def fused_run(pkg, dev, W, B, launches, seed, id0, eps, lr, gamma, boards=None):
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    agent = pkg.BatchedRowTupleAgent(100, learning_rate=lr, discount_factor=gamma, exploration_rate=eps, seed=seed,
                                     env_id0=id0, device=dev)
    agent.weights.copy_(torch.from_numpy(W))
    if boards is not None:
        env.boards.copy_(torch.from_numpy(boards))
    for k in launches:
        agent.fused_rollout(env, k)
    assert agent.check_status() == 0
    return env, agent


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B,steps,eps", [(257, 200, 0.3), (1000, 120, 0.0)])
def test_fused_rollout_with_frozen_weights(pkg, O, dev, B, steps, eps):
    """learning_rate = 0: every lane is a function of W alone, so the sequential oracle is the specification at any
    batch size.  Launches of 1 and steps - 1 steps: the entries carried from step to step, the entries gathered again
    after a reset and the first gather of a launch all decide actions here.  Boards, aux records and statistics equal
    the oracle's; the weights are bit for bit what was loaded.  Teeth: on zero weights the same run ends on other
    boards in more than half of the lanes (CPU twin: 257 of 257 and 996 of 1000)."""
    seed, id0, gamma = 17, 1000, 0.97
    W = (0.5 * np.random.default_rng(500 + B).standard_normal((4, 65536, 4))).astype(F32)
    envs = O.envs_init(B, 4, seed, id0)
    oa = O.RowTupleAgent(0.0, gamma, eps)
    oa.set_weights(W)
    si, sf = oa.rollout(envs, steps, seed, id0, 0)
    assert_same_bits(oa.weights(), W, "the oracle's weights moved at learning rate 0")

    env, agent = fused_run(pkg, dev, W, B, (1, steps - 1), seed, id0, eps, 0.0, gamma)
    boards = env.boards.cpu().numpy()
    assert np.array_equal(boards, envs["board"][:, :16]), \
        f"boards differ on {int((boards != envs['board'][:, :16]).any(axis=1).sum())} of {B} lanes"
    assert_aux(env.aux_fields(), envs, f"B = {B}")
    st = agent.stats()
    assert st["steps"] == B * steps == si[O.ST_STEPS]
    assert st["episodes"] == si[O.ST_EPISODES] and st["episodes"] > 0       # resets happened
    assert st["valid_moves"] == si[O.ST_VALID] and st["explored"] == si[O.ST_EXPLORE]
    assert st["score_sum"] == si[O.ST_SCORE]
    assert (st["explored"] == 0) == (eps == 0.0)
    assert_same_bits(agent.weights, W, "frozen weights were written")

    env0, _ = fused_run(pkg, dev, np.zeros_like(W), B, (1, steps - 1), seed, id0, eps, 0.0, gamma)
    differ = int((env0.boards.cpu().numpy() != boards).any(axis=1).sum())
    assert differ > B // 2, f"the weights decide the boards of only {differ} of {B} lanes"


# ---------------------------------------------------------------------------------------------------------------
# 6. fused rollout, one learning step on rows that cannot race
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [65, 257, 1000])
def test_fused_rollout_one_learning_step(pkg, O, dev, B):
    """One step with gamma = 0, lr = 0.1, epsilon = 0.3 from boards whose row indices are, per row position, distinct
    across lanes (cells 0..11, a slice of a permutation of 12^4).  With gamma = 0 the step size does not read s', and
    the entries of s are private to the lane, so the sequential oracle is the specification.  Boards and aux records
    after the step equal the oracle's and the whole weight array equals the oracle's bit for bit: 4 B entries changed.
    The only exact check of rt_scatter inside the fused loop at B > 1."""
    seed, id0, eps, lr, gamma = 23, 4000, 0.3, 0.1, 0.0
    rng = np.random.default_rng(600 + B)
    W = (0.5 * rng.standard_normal((4, 65536, 4))).astype(F32)
    digits = np.stack([rng.permutation(12 ** 4)[:B] for _ in range(4)], axis=1)               # [B, 4], base 12
    boards = np.stack([(digits[:, r] // 12 ** k) % 12 for r in range(4) for k in range(4)], axis=1).astype(np.uint8)
    idx = model_idx(boards)
    assert boards.max() == 11 and all(len(np.unique(idx[:, r])) == B for r in range(4))

    envs = O.envs_init(B, 4, seed, id0)
    envs["board"][:, :16] = boards
    oa = O.RowTupleAgent(lr, gamma, eps)
    oa.set_weights(W)
    si, _ = oa.rollout(envs, 1, seed, id0, 0)
    want = oa.weights()
    assert int((bits(want) != bits(W)).sum()) == 4 * B
    assert 0 < si[O.ST_EXPLORE] < B

    env, agent = fused_run(pkg, dev, W, B, (1,), seed, id0, eps, lr, gamma, boards=boards)
    assert np.array_equal(env.boards.cpu().numpy(), envs["board"][:, :16])
    assert_aux(env.aux_fields(), envs, f"B = {B}")
    got = agent.weights.cpu().numpy()
    assert_same_bits(got, want, f"B = {B}")
    assert int((bits(got) != bits(W)).sum()) == 4 * B
    st = agent.stats()
    assert st["steps"] == B and st["explored"] == si[O.ST_EXPLORE] and st["valid_moves"] == si[O.ST_VALID]


# ---------------------------------------------------------------------------------------------------------------
# 7. the argument checks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_argument_checks(pkg, dev):
    """The codes q2048_kernels.hip and q2048_host.cpp return, in their order of precedence (batch size, NULL,
    alignment, steps, scalar ranges), on both libraries: a NULL in every required pointer position, B = -1, a B one
    above what the grid holds, every 16-byte-aligned pointer off by 8 bytes, epsilon outside [0, 1] or NaN, lr or gamma
    NaN, steps negative or above 2^30.  (stats_i and stats_f of the fused rollout are optional, the stream is the
    default stream when NULL.)  B = 0 and steps = 0 return 0.  No such call writes a canaried output, an input or the
    weights."""
    L, B, nan = lib(pkg, dev), 4, float("nan")
    rng = np.random.default_rng(7)
    W = t32(dev, base_weights())
    boards, boards2 = t8(dev, random_boards(rng, B + 1)), t8(dev, random_boards(rng, B + 1))
    env_boards = torch.zeros((B + 1, 16), dtype=torch.uint8, device=dev)
    aux = torch.zeros((B + 1, 16), dtype=torch.uint8, device=dev)
    assert L.q2048_env_init(env_boards.data_ptr(), aux.data_ptr(), B, 4, 3, 50, None) == 0
    actions_out = torch.full((B + ROOM,), A_CANARY, dtype=torch.uint8, device=dev)
    q_out = torch.full((B + ROOM, 4), Q_CANARY - (1 << 32), dtype=torch.int32, device=dev)
    actions = t8(dev, rng.integers(0, 4, size=B))
    reward, done = t32(dev, rng.standard_normal(B)), t8(dev, rng.integers(0, 2, size=B))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stats_i = torch.zeros(pkg._native.NSTAT_I, dtype=torch.int64, device=dev)
    stats_f = torch.zeros(pkg._native.NSTAT_F, dtype=torch.float64, device=dev)
    buffers = [W, boards, boards2, env_boards, aux, actions_out, q_out, actions, reward, done, status, stats_i, stats_f]
    before = [t.clone() for t in buffers]

    def untouched(what):
        for k, (t, b) in enumerate(zip(buffers, before)):
            assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), f"{what}: buffer {k} was written"

    p = lambda t: t.data_ptr()  # noqa: E731
    # (function, good arguments, required pointers, 16-byte aligned pointers, B, {scalar position: refused values})
    entry_points = {
        "rt_choose": (L.q2048_rt_choose, [p(W), p(boards), B, 0.3, 7, 50, 3, p(actions_out), None],
                      (0, 1, 7), (0, 1), 2, {3: (-0.1, 1.5, nan)}),
        "rt_lookup": (L.q2048_rt_lookup, [p(W), p(boards), B, p(q_out), None], (0, 1, 3), (0, 1, 3), 2, {}),
        "rt_update": (L.q2048_rt_update, [p(W), p(boards), p(actions), p(reward), p(boards2), p(done), B, 0.1, 0.97,
                                          p(status), None],
                      (0, 1, 2, 3, 4, 5, 9), (0, 1, 4), 6, {7: (nan,), 8: (nan,)}),
        "rt_fused_rollout": (L.q2048_rt_fused_rollout, [p(env_boards), p(aux), p(W), B, 2, 0.3, 0.1, 0.97, 3, 50, 0,
                                                        p(stats_i), p(stats_f), p(status), None],
                             (0, 1, 2, 13), (0, 1, 2), 3, {5: (-0.1, 1.5, nan), 6: (nan,), 7: (nan,)}),
    }
    for name, (fn, good, pointers, aligned, b_pos, scalars) in entry_points.items():
        def call(pos, value):
            args = list(good)
            args[pos] = value
            return fn(*args)

        for pos in pointers:
            assert call(pos, None) == ERR_NULL, f"{name}: NULL in position {pos}"
            untouched(f"{name}: NULL in position {pos}")
        for pos in aligned:
            assert call(pos, good[pos] + 8) == ERR_ALIGN, f"{name}: position {pos} off by 8 bytes"
            untouched(f"{name}: position {pos} off by 8 bytes")
        for value in (-1, GRID_LIMIT + 1):
            assert call(b_pos, value) == ERR_SIZE, f"{name}: B = {value}"
            untouched(f"{name}: B = {value}")
        for pos, values in scalars.items():
            for value in values:
                assert call(pos, value) == ERR_RANGE, f"{name}: {value} in position {pos}"
                untouched(f"{name}: {value} in position {pos}")
        assert call(b_pos, 0) == 0, f"{name}: B = 0"
        untouched(f"{name}: B = 0")
    fn, good = entry_points["rt_fused_rollout"][:2]
    for steps, code in ((-1, ERR_SIZE), ((1 << 30) + 1, ERR_SIZE), (0, 0)):
        args = list(good)
        args[4] = steps
        assert fn(*args) == code, f"rt_fused_rollout: steps = {steps}"
        untouched(f"rt_fused_rollout: steps = {steps}")
    # precedence: the batch size before a NULL, a NULL before the alignment, steps before epsilon
    assert L.q2048_rt_lookup(None, p(boards), -1, p(q_out), None) == ERR_SIZE
    assert L.q2048_rt_lookup(None, p(boards) + 8, B, p(q_out), None) == ERR_NULL
    args = list(good)
    args[4], args[5] = -1, nan
    assert fn(*args) == ERR_SIZE
    untouched("precedence")
    # and the good arguments are good: without the optional statistics, two steps on four boards
    args = list(good)
    args[11] = args[12] = None
    assert fn(*args) == 0
    assert int(status.item()) == 0 and torch.equal(stats_i, before[11]) and torch.equal(stats_f, before[12])
    assert not torch.equal(W, before[0]) and not torch.equal(env_boards[:B], before[3][:B])
    assert torch.equal(env_boards[B:], before[3][B:]) and torch.equal(aux[B:], before[4][B:])
