"""Carousel shaping for the staged network (q2048_car_fused_rollout, q2048_car_commit) against a numpy model of the
contract "CAROUSEL SHAPING" in q2048_core.hpp, on the CPU twin and on the device.  (The scripts and the checkpoint:
test_carousel_scripts.py.)

Which test executes which kernel (device) / function (CPU twin):
  the argument checks      test_abi, test_argument_errors_in_order, test_refused_calls_write_nothing
  k_car_commit             test_commit_against_the_model, test_commit_edges
  k_car_fused_rollout      test_empty_pool_is_the_staged_learner, test_one_lane_with_commits,
                           test_many_lanes_at_fixed_weights, test_racing_lanes_at_65536_boards_properties

Every comparison is exact, byte for byte (weights: float32 bit patterns).  The learner's model is the four-call loop of a
second agent -- choose_action / env.step / update_q_value / env.reset -- with the recording and restart rules applied in
Python between the calls; the restart's slot comes from the oracle's reset draws."""
import subprocess

import numpy as np
import pytest
import torch

import test_ntuple as NT
import test_ntuple_stages as ST
import test_row_tuple_kernels as K
import test_row_tuple_player as RP

REPO, DEVICES, F32, NIDX = NT.REPO, NT.DEVICES, NT.F32, NT.NIDX
ERR_NULL, ERR_SIZE, ERR_ALIGN, ERR_RANGE = NT.ERR_NULL, NT.ERR_SIZE, NT.ERR_ALIGN, NT.ERR_RANGE
lib, t8, t32, bits, assert_same_bits = NT.lib, NT.t8, NT.t32, NT.bits, NT.assert_same_bits
spec, tables, tables_on, model_stage, make_agent = ST.spec, ST.tables, ST.tables_on, ST.model_stage, ST.make_agent
NAMES = ("q2048_car_fused_rollout", "q2048_car_commit")
CANARY = 0xC7


# ---------------------------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------------------------
def model_commit(pool, counts, fresh, P):
    """The commit on numpy arrays, in place: pool uint8 [S, P, 32], counts uint64 [S], fresh uint8 [S, B, 32]."""
    for k in range(1, pool.shape[0]):
        lanes = np.flatnonzero(fresh[k, :, :16].any(axis=1))          # ascending
        m = len(lanes)
        for r, i in enumerate(lanes):
            if r + P >= m:
                pool[k, (int(counts[k]) + r) % P] = fresh[k, i]
            fresh[k, i] = 0
        counts[k] += np.uint64(m)


def record(board, aux_row):
    """board uint8 [16], aux_row uint8 [16] -> the 32 bytes of a record"""
    rec = np.zeros(32, np.uint8)
    rec[:16], rec[16:24] = board, aux_row[:8]
    return rec


def car_buffers(dev, pool, counts, B):
    """device copies of a numpy pool and counts, and a zero `fresh` for B lanes"""
    S_ = pool.shape[0]
    return (t8(dev, pool), torch.from_numpy(counts.astype(np.int64)).to(dev),
            torch.zeros((S_, B, 32), dtype=torch.uint8, device=dev))


def u64(t):
    return t.cpu().numpy().view(np.uint64)


class Tally:
    def __init__(self, S_):
        self.from_pool, self.fallback, self.overwritten, self.recorded = [0] * S_, 0, 0, [0] * S_

    def assert_presence(self):
        print(f"restarts from the pool per stage {self.from_pool}, resets on an empty pool {self.fallback}, records "
              f"overwritten within a launch {self.overwritten}, records written per stage {self.recorded}")
        assert self.from_pool[1] >= 3 and self.from_pool[2] >= 3 and self.fallback >= 1 and self.overwritten >= 1


def model_launch(O, dev, loop, env, thr, pool, counts, P, steps, learn, tally):
    """`steps` steps of the four-call loop on `env` with the recording and restart rules applied in Python; the pool and
    the counts (numpy) are only read.  -> fresh uint8 [S, B, 32] as the launch leaves it (from zero)."""
    S_, B = len(thr) + 1, env.num_envs
    fresh = np.zeros((S_, B, 32), np.uint8)
    for _ in range(steps):
        s = env.boards.cpu().numpy().copy()
        a = loop.choose_action(env.boards)
        s2, r, done, _ = env.step(a)
        if learn:
            loop.update_q_value(t8(dev, s), a, r, s2, done)
        s2n, dn, aux = s2.cpu().numpy().copy(), done.cpu().numpy().astype(bool), env.aux.cpu().numpy()
        k0, k1 = model_stage(s, thr), model_stage(s2n, thr)
        for i in np.flatnonzero(~dn & (k1 > k0)):
            tally.overwritten += bool(fresh[k1[i], i, :16].any())
            tally.recorded[k1[i]] += 1
            fresh[k1[i], i] = record(s2n[i], aux[i])
        env.reset(done)
        if not dn.any():
            continue
        boards, aux, took = env.boards.cpu().numpy().copy(), env.aux.cpu().numpy().copy(), False
        for i in np.flatnonzero(dn):
            episode = int(aux[i, 12:16].view(np.uint32)[0])
            k = episode % S_
            n = min(int(counts[k]), P) if k else 0
            if n == 0:
                tally.fallback += k != 0
                continue
            x0 = int(O.draws(env.seed, env.env_id0 + int(i), episode, O.STREAM_RESET)[0])
            rec = pool[k, (x0 * n) >> 32]
            boards[i], aux[i, :8], took = rec[:16], rec[16:24], True
            tally.from_pool[k] += 1
        if took:
            env.boards.copy_(torch.from_numpy(boards))
            env.aux.copy_(torch.from_numpy(aux))
    return fresh


def full_board(pair, rest=(1, 2)):
    """A full board without equal neighbours except one horizontal pair of `pair` in the top row: the only moves are
    left and right, both merge the pair; what follows has two or three empty cells and ends within a few moves."""
    b = np.array([rest[(r + c) & 1] for r in range(4) for c in range(4)], np.uint8)
    b[0], b[1] = pair, pair
    return b


def filled_pool(S_, P, rows):
    """pool and counts with `rows[k]` = the boards of stage k's first slots; scores and returns that tell the slots apart"""
    pool, counts = np.zeros((S_, P, 32), np.uint8), np.zeros(S_, np.uint64)
    for k, boards in rows.items():
        for j, b in enumerate(boards):
            pool[k, j, :16] = b
            pool[k, j, 16:20] = np.array([1000 * k + 4 * j], np.int32).view(np.uint8)
            pool[k, j, 20:24] = np.array([0.5 * k + j], F32).view(np.uint8)
        counts[k] = len(boards)
    return pool, counts


# ---------------------------------------------------------------------------------------------------------------
# 1. ABI and argument checks
# ---------------------------------------------------------------------------------------------------------------
def test_abi(pkg):
    N = pkg._native
    with open(f"{REPO}/include/q2048.h") as fh:
        header = fh.read()
    for path in (N.LIB_PATH, N.HOST_LIB_PATH):
        exported = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
        assert {n for n in exported if n.startswith("q2048_car_")} == set(NAMES), path
    assert {n for n in N._SIGNATURES if n.startswith("q2048_car_")} == set(NAMES)
    for name in NAMES:
        assert hasattr(N.host_lib(), name) and hasattr(N.lib(), name), name
        assert f"int {name}(" in header, name
    C = __import__("ctypes")
    res, args = N._SIGNATURES["q2048_nts_fused_rollout"]      # pool, counts, fresh and P after `stages`
    assert N._SIGNATURES["q2048_car_fused_rollout"] == (res, args[:4] + [C.c_void_p] * 3 + [C.c_int64] + args[4:])
    assert N.host_lib().q2048_abi_version() == 7 == N.lib().q2048_abi_version() == N.ABI_VERSION     # the number stays


@pytest.mark.parametrize("which", ["hip", "host"])
def test_argument_errors_in_order(pkg, which):
    """One call per error, each with every LATER check failing too: the spec, NULLs, alignment, then P, B, steps and the
    scalars.  Made-up addresses: nothing behind them is touched, so no device is needed."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    nan, g = float("nan"), spec(3, 6)
    bo, au, w, po, co, fr, stt = (0x10000 * (k + 2) for k in range(7))

    def fused(boards=bo, aux=au, weights=w, stages=g, pool=po, counts=co, fresh=fr, P=4, B=64, steps=2, eps=0.3, lr=0.1,
              gamma=0.9, status=stt):
        return L.q2048_car_fused_rollout(boards, aux, weights, stages, pool, counts, fresh, P, B, steps, eps, lr, gamma, 1,
                                         0, 0, None, None, status, None)

    def commit(pool=po, counts=co, fresh=fr, stages=g, P=4, B=64):
        return L.q2048_car_commit(pool, counts, fresh, stages, P, B, None)

    for what, bad in ST.BAD_SPECS.items():
        assert fused(stages=bad) == ERR_RANGE and commit(stages=bad) == ERR_RANGE, what
        assert fused(stages=bad, boards=None, aux=au + 8, P=0, B=-1, steps=-1, eps=nan) == ERR_RANGE, what
        assert commit(stages=bad, pool=None, fresh=fr + 8, P=0, B=-1) == ERR_RANGE, what
    later = dict(P=0, B=-1, steps=-1, eps=nan, lr=nan, gamma=nan)
    for name in ("boards", "aux", "weights", "pool", "counts", "fresh", "status"):
        assert fused(**{name: None}) == ERR_NULL, name
        other = "aux" if name != "aux" else "boards"
        assert fused(**{name: None, other: 0x20008}, **later) == ERR_NULL, f"{name}: NULL before alignment and sizes"
    for name in ("pool", "counts", "fresh"):
        assert commit(**{name: None}) == ERR_NULL and commit(**{name: None}, P=0, B=-1) == ERR_NULL, name
    for name, addr in (("boards", bo), ("aux", au), ("weights", w), ("pool", po), ("fresh", fr)):
        assert fused(**{name: addr + 8}) == ERR_ALIGN, name
        assert fused(**{name: addr + 8}, **later) == ERR_ALIGN, f"{name}: alignment before sizes and scalars"
    assert fused(counts=co + 4) == ERR_ALIGN and fused(counts=co + 8, steps=0) == 0      # counts: 8 bytes
    for name, addr in (("pool", po), ("fresh", fr)):
        assert commit(**{name: addr + 8}) == ERR_ALIGN and commit(**{name: addr + 8}, P=0, B=-1) == ERR_ALIGN, name
    assert commit(counts=co + 4) == ERR_ALIGN and commit(counts=co + 4, P=0) == ERR_ALIGN
    for P in (0, -1, (1 << 32) + 1):
        assert fused(P=P) == ERR_SIZE and fused(P=P, eps=nan, lr=nan) == ERR_SIZE and commit(P=P) == ERR_SIZE, P
    assert fused(B=-1) == ERR_SIZE and fused(B=-1, eps=nan) == ERR_SIZE and commit(B=-1) == ERR_SIZE
    assert fused(steps=-1) == ERR_SIZE and fused(steps=-1, gamma=nan) == ERR_SIZE
    for kw in (dict(eps=nan), dict(eps=-0.1), dict(eps=1.5), dict(lr=nan), dict(gamma=nan)):
        assert fused(**kw) == ERR_RANGE, kw
    # B == 0 and steps == 0 are no-ops behind the checks; so is a commit at S = 1
    assert fused(B=0) == 0 and fused(steps=0) == 0 and commit(B=0) == 0 and commit(stages=0) == 0
    assert fused(stages=0, steps=0) == 0


@pytest.mark.parametrize("dev", DEVICES)
def test_refused_calls_write_nothing(pkg, dev):
    """Both entry points refused for a malformed spec and for their LAST check under a good spec, on real buffers; and
    the Q2048_OK calls with B == 0 and steps == 0: every byte of every buffer stays."""
    L, B, P, nan, g, bad = lib(pkg, dev), 64, 4, float("nan"), spec(3, 6), spec(5, 3)
    W = tables_on(dev, 3)
    boards = t8(dev, K.random_boards(np.random.default_rng(1), B))
    aux = torch.full((B, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    pool = torch.full((3, P, 32), CANARY, dtype=torch.uint8, device=dev)
    counts = torch.full((3,), 2, dtype=torch.int64, device=dev)
    fresh = torch.full((3, B, 32), CANARY, dtype=torch.uint8, device=dev)
    si, sf = torch.full((64,), 7, dtype=torch.int64, device=dev), torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((1,), 0x777, dtype=torch.int32, device=dev)
    everything = (boards, aux, pool, counts, fresh, si, sf, status)
    before = [t.clone() for t in everything]
    p = lambda t: t.data_ptr()      # noqa: E731

    def fused(stages=g, P_=P, B_=B, steps=3, lr=0.1):
        return L.q2048_car_fused_rollout(p(boards), p(aux), p(W), stages, p(pool), p(counts), p(fresh), P_, B_, steps, 0.3,
                                         lr, 0.9, 1, 0, 0, p(si), p(sf), p(status), None)

    assert fused(stages=bad) == ERR_RANGE and fused(lr=nan) == ERR_RANGE and fused(P_=0) == ERR_SIZE
    assert L.q2048_car_commit(p(pool), p(counts), p(fresh), bad, P, B, None) == ERR_RANGE
    assert L.q2048_car_commit(p(pool), p(counts), p(fresh), g, 0, B, None) == ERR_SIZE
    assert L.q2048_car_commit(p(pool), p(counts), p(fresh), g, P, -1, None) == ERR_SIZE
    assert fused(B_=0) == 0 and fused(steps=0) == 0
    assert L.q2048_car_commit(p(pool), p(counts), p(fresh), g, P, 0, None) == 0
    RP.sync(dev)
    for t, b in zip(everything, before):
        assert torch.equal(t, b), "a refused or empty call wrote something"
    ST.assert_tables_unwritten(dev, 3, "a refused call wrote to the weights")


# ---------------------------------------------------------------------------------------------------------------
# 2. the commit against the numpy model
# ---------------------------------------------------------------------------------------------------------------
def fresh_pattern(rng, name, S_, B):
    """fresh uint8 [S, B, 32] with non-empty records where `name` says, each stage with lanes of its own where random.
    A non-empty record has random bytes everywhere -- 24..31 included: the commit moves all 32 -- and a tile in cell 0."""
    has = np.zeros((S_, B), bool)
    if name == "all":
        has[:] = True
    elif name == "last":
        has[:, B - 1] = True
    elif name == "every64":
        has[:, ::64] = True
    elif name == "random":
        has = rng.random((S_, B)) < 0.4
    fresh = rng.integers(0, 256, (S_, B, 32)).astype(np.uint8)
    fresh[:, :, 0] |= 1
    fresh[~has, :16] = 0                 # empty: the board is zero; what the other 16 bytes hold does not matter
    return fresh


def run_commit(pkg, dev, pool, counts, fresh, P, times=1, refill=None):
    """The library's commit beside the model's on copies; -> nothing, asserts every byte of the three buffers"""
    L, (S_, B) = lib(pkg, dev), fresh.shape[:2]
    tp, tc, tf = t8(dev, pool), torch.from_numpy(counts.view(np.int64).copy()).to(dev), t8(dev, fresh)
    pool, counts, fresh = pool.copy(), counts.copy(), fresh.copy()
    for n in range(times):
        if n and refill is not None:
            fresh[:] = refill
            tf.copy_(torch.from_numpy(refill))
        assert L.q2048_car_commit(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), spec(*range(1, S_)), P, B, None) == 0
        model_commit(pool, counts, fresh, P)
        RP.sync(dev)
        what = f"B = {B}, P = {P}, commit {n}"
        assert np.array_equal(u64(tc), counts), what
        assert np.array_equal(tp.cpu().numpy(), pool), what
        assert np.array_equal(tf.cpu().numpy(), fresh), what
    return pool, counts, fresh


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_commit_against_the_model(pkg, dev, B):
    """S = 3, every P of (1, 3, 64, 1000) with every pattern of fresh records, the counts starting at 0, at P - 1 and
    far past P (the ring wraps; a count beyond 2^32 too), two commits in a row (the second on new records).  Exact on
    every byte of pool, counts and fresh; row 0 of the pool and of fresh, and the slots no record lands in, keep their
    canaries."""
    rng, S_ = np.random.default_rng(B), 3
    for P in (1, 3, 64, 1000):
        for name in ("none", "all", "last", "every64", "random"):
            for start in (0, P - 1, 5 * P + 2, (1 << 33) + 7):
                pool = np.full((S_, P, 32), CANARY, np.uint8)
                counts = np.array([99, start, start + 1], np.uint64)
                fresh = fresh_pattern(rng, name, S_, B)
                again = fresh_pattern(rng, "random", S_, B)
                again[0] = fresh[0]
                got_pool, got_counts, got_fresh = run_commit(pkg, dev, pool, counts, fresh, P, times=2, refill=again)
                assert (got_pool[0] == CANARY).all() and got_counts[0] == 99, "row 0 of the pool or its count was written"
                assert np.array_equal(got_fresh[0], fresh[0]), "row 0 of fresh was written"
                m = int(fresh[1, :, :16].any(axis=1).sum()) + int(again[1, :, :16].any(axis=1).sum())
                assert int(got_counts[1]) == start + m
                if name == "none" and P == 1000:
                    assert m <= P or B > P


@pytest.mark.parametrize("dev", DEVICES)
def test_commit_edges(pkg, dev):
    """m == P and m == P + 1 exactly (the first record of P + 1 is dropped, every slot is written once), the landing
    order at a wrap, and bytes 24..31: the learner's records hold zero there and the pool then does too; an empty record
    with stray bytes in its second half is not consumed and not changed."""
    S_, P = 3, 64
    for m, B in ((P, 200), (P + 1, 200), (P + 1, P + 1), (1025 + P, 2049)):
        fresh = np.zeros((S_, B, 32), np.uint8)
        lanes = np.sort(np.random.default_rng(m + B).choice(B, m, replace=False))
        for k in (1, 2):
            fresh[k, lanes, 0] = 1 + (np.arange(m) % 11)
            fresh[k, lanes, 16:20] = np.arange(m, dtype=np.int32)[:, None].view(np.uint8).reshape(m, 4)   # the rank, as the score
        stray = [i for i in range(B) if i not in set(lanes.tolist())][:1]
        fresh[1, stray, 20] = 9                                              # an EMPTY record: board zero
        pool = np.full((S_, P, 32), CANARY, np.uint8)
        counts = np.array([0, 10, 0], np.uint64)
        got_pool, got_counts, got_fresh = run_commit(pkg, dev, pool, counts, fresh, P)
        ranks = got_pool[1, :, 16:20].copy().view(np.int32).ravel()
        assert sorted(ranks.tolist()) == list(range(m - P, m)), "the last P records land, each in a slot of its own"
        assert all(ranks[(10 + r) % P] == r for r in range(m - P, m))
        assert (got_pool[1:, :, 24:] == 0).all() and int(got_counts[1]) == 10 + m
        if stray:
            assert got_fresh[1, stray[0], 20] == 9 and not got_fresh[1, lanes].any()


# ---------------------------------------------------------------------------------------------------------------
# 3. an empty pool is the staged learner
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_empty_pool_is_the_staged_learner(pkg, O, dev):
    """B = 1, 300 steps in launches of 1, 63 and 236, thresholds (3, 6) as in test_one_lane_300_steps, P = 4 and NO commit
    between the launches: the pool stays empty, every restart is a reset, and boards, aux, statistics and all 768 MiB
    equal q2048_nts_fused_rollout's bit for bit.  `fresh` equals the records the model takes from the four-call loop
    (the last crossing into a stage wins over all three launches).  stages == 0 gives the staged learner's bytes too."""
    L, seed, id0, eps, lr, gamma, cuts, thr, P = lib(pkg, dev), 5, 77, 0.3, 0.1, 0.97, (1, 63, 236), (3, 6), 4
    g = spec(*thr)

    def run(car, stages, S_):
        W = t32(dev, tables(S_))
        env = pkg.BatchedGame2048Env(1, seed=seed, env_id0=id0, device=dev)
        si, sf = torch.zeros(64, dtype=torch.int64, device=dev), torch.zeros(16, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        pool, counts, fresh = car_buffers(dev, np.zeros((S_, P, 32), np.uint8), np.zeros(S_, np.uint64), 1)
        ctr = 0
        for c in cuts:
            head = (env.boards.data_ptr(), env.aux.data_ptr(), W.data_ptr(), stages)
            tail = (1, c, eps, lr, gamma, seed, id0, ctr, si.data_ptr(), sf.data_ptr(), status.data_ptr(), None)
            if car:
                assert L.q2048_car_fused_rollout(*head, pool.data_ptr(), counts.data_ptr(), fresh.data_ptr(), P, *tail) == 0
            else:
                assert L.q2048_nts_fused_rollout(*head, *tail) == 0
            ctr += c
        RP.sync(dev)
        assert not pool.any() and not counts.any() and int(status.item()) == 0
        return env.boards.cpu(), env.aux.cpu(), si.cpu(), sf.cpu(), W, fresh.cpu().numpy()

    want, got = run(False, g, 3), run(True, g, 3)
    assert all(torch.equal(a, b) for a, b in zip(got[:4], want[:4])), "boards, aux or statistics differ"
    assert_same_bits(got[4], want[4], "an empty pool: all three tables")
    want, got = None, got[:4] + got[5:]              # (the tables go; got[4] is fresh now)
    # the records: the model's, from the four-call loop of the staged agent (no pool: every restart is a reset)
    env_l = pkg.BatchedGame2048Env(1, seed=seed, env_id0=id0, device=dev)
    loop = make_agent(pkg, dev, (8, 64), eps, lr, gamma, seed, id0, weights=t32(dev, tables(3)))
    tally, fresh = Tally(3), np.zeros((3, 1, 32), np.uint8)
    for c in cuts:
        new = model_launch(O, dev, loop, env_l, thr, np.zeros((3, P, 32), np.uint8), np.zeros(3, np.uint64), P, c, True, tally)
        fresh = np.where(new[:, :, :16].any(axis=2, keepdims=True), new, fresh)
    assert torch.equal(env_l.boards.cpu(), got[0]) and torch.equal(env_l.aux.cpu(), got[1])
    assert tally.recorded[1] >= 1 and tally.recorded[2] >= 1 and sum(tally.from_pool) == 0
    assert np.array_equal(got[4], fresh), "fresh differs from the model's records"
    del loop, got
    want, got = run(False, 0, 1), run(True, 0, 1)
    assert all(torch.equal(a, b) for a, b in zip(got[:4], want[:4])), "stages == 0: boards, aux or statistics differ"
    assert_same_bits(got[4], want[4], "stages == 0")
    assert not got[5].any(), "stages == 0 recorded something"


# ---------------------------------------------------------------------------------------------------------------
# 4. one lane, with commits: the full exact test
# ---------------------------------------------------------------------------------------------------------------
ONE_LANE = dict(seed=5, id0=77, cuts=(1, 63, 236, 500, 700), P=4)


def one_lane_pool():
    """Stage 1 hand-filled with three full boards whose only moves merge two 32s (the game enters stage 2 = tile 64 on
    the spot and ends a few moves later); stage 2 empty: its first turn falls back to a reset, later ones draw from what
    the commits brought."""
    return filled_pool(3, ONE_LANE["P"], {1: [full_board(5), full_board(5, (2, 3)), full_board(5, (1, 3))]})


@pytest.mark.parametrize("dev", DEVICES)
def test_one_lane_with_commits(pkg, O, dev):
    """B = 1 through the agent (carousel = 4, learning at epsilon 0.3, thresholds (3, 6)), launches of 1, 63, 236, 500
    and 700 steps with the commit after each, against a second agent's four-call loop with the restart and recording
    rules applied in Python.  Weights (768 MiB), boards, aux, pool and counts bit for bit at the end; boards, aux, pool
    and counts at every launch boundary.  The model run itself restarts at least 3 times from the pool into each of
    stages 1 and 2, falls back to a reset on an empty pool and overwrites a record within a launch."""
    seed, id0, cuts, P = (ONE_LANE[k] for k in ("seed", "id0", "cuts", "P"))
    eps, lr, gamma, tiles, thr = 0.3, 0.1, 0.97, (8, 64), (3, 6)
    pool, counts = one_lane_pool()
    env_l = pkg.BatchedGame2048Env(1, seed=seed, env_id0=id0, device=dev)
    loop = make_agent(pkg, dev, tiles, eps, lr, gamma, seed, id0, weights=t32(dev, tables(3)))
    env = pkg.BatchedGame2048Env(1, seed=seed, env_id0=id0, device=dev)
    agent = pkg.BatchedNTupleAgent(100, learning_rate=lr, discount_factor=gamma, exploration_rate=eps, seed=seed,
                                   env_id0=id0, device=dev, stage_tiles=tiles, carousel=P)
    agent.weights = t32(dev, tables(3))
    agent.carousel_pool.copy_(torch.from_numpy(pool))
    agent.carousel_counts.copy_(torch.from_numpy(counts.view(np.int64)))
    tally = Tally(3)
    for n, c in enumerate(cuts):
        fresh = model_launch(O, dev, loop, env_l, thr, pool, counts, P, c, True, tally)
        model_commit(pool, counts, fresh, P)
        agent.fused_rollout(env, c)
        RP.sync(dev)
        assert torch.equal(env.boards.cpu(), env_l.boards.cpu()) and torch.equal(env.aux.cpu(), env_l.aux.cpu()), f"launch {n}"
        assert np.array_equal(agent.carousel_pool.cpu().numpy(), pool), f"the pool after launch {n}"
        assert np.array_equal(u64(agent.carousel_counts), counts), f"the counts after launch {n}"
        assert not agent.carousel_fresh.any(), "the commit left a record in fresh"
    tally.assert_presence()
    assert agent.check_status() == 0 and loop.check_status() == 0
    assert agent.stats()["steps"] == sum(cuts)
    assert agent.carousel_summary() == {"counts": [int(c) for c in counts], "valid": [min(int(c), P) for c in counts]}
    assert_same_bits(agent.weights, loop.weights, "one lane with commits, all three tables")


# ---------------------------------------------------------------------------------------------------------------
# 5. many lanes at fixed weights
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [63, 64, 65, 257])
def test_many_lanes_at_fixed_weights(pkg, O, dev, B):
    """lr = 0, epsilon = 0.3, random distinct tables, thresholds (3, 5) = tiles (8, 32), 200 steps in 4 launches with the
    commit after each, P = 16.  Row 1 of the pool starts hand-filled with full stage-1 boards whose only moves merge two
    16s -- the game enters stage 2 on the spot and ends a few moves later -- and two lanes in three start on full boards
    too, so that restarts, crossings and overwritten records are frequent; row 2 starts empty (its turns of the first
    launch fall back to a reset) and is filled by the commits.  At lr = 0 the TD step writes back the bits it gathered, so the lanes do not interact:
    boards, aux, fresh (before each commit), pool and counts are exact at every launch boundary, and the weights stay
    what they were bit for bit."""
    L, seed, id0, eps, gamma, thr, tiles, P, cuts = lib(pkg, dev), 11, 300, 0.3, 0.9, (3, 5), (8, 32), 16, (50, 50, 50, 50)
    g, S_ = spec(*thr), 3
    pool, counts = filled_pool(S_, P, {1: [full_board(4, rest) for rest in ((1, 2), (2, 3), (1, 3), (2, 1), (3, 1))]})
    W = tables_on(dev, S_)
    env_l = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    start = np.stack([full_board(1 + i % 4, (5, 6)) if i % 3 else env.boards[i].cpu().numpy() for i in range(B)])
    for e in (env, env_l):
        e.boards.copy_(torch.from_numpy(start))
    loop = make_agent(pkg, dev, tiles, eps, 0.0, gamma, seed, id0, weights=W)
    tp, tc, tf = car_buffers(dev, pool, counts, B)
    si, sf = torch.zeros(64, dtype=torch.int64, device=dev), torch.zeros(16, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    tally, ctr = Tally(S_), 0
    for n, c in enumerate(cuts):
        fresh = model_launch(O, dev, loop, env_l, thr, pool, counts, P, c, False, tally)
        assert L.q2048_car_fused_rollout(env.boards.data_ptr(), env.aux.data_ptr(), W.data_ptr(), g, tp.data_ptr(),
                                         tc.data_ptr(), tf.data_ptr(), P, B, c, eps, 0.0, gamma, seed, id0, ctr,
                                         si.data_ptr(), sf.data_ptr(), status.data_ptr(), None) == 0
        RP.sync(dev)
        what = f"B = {B}, launch {n}"
        assert torch.equal(env.boards.cpu(), env_l.boards.cpu()) and torch.equal(env.aux.cpu(), env_l.aux.cpu()), what
        assert np.array_equal(tf.cpu().numpy(), fresh), f"{what}: fresh"
        assert np.array_equal(tp.cpu().numpy(), pool) and np.array_equal(u64(tc), counts), f"{what}: the learner wrote the pool"
        assert L.q2048_car_commit(tp.data_ptr(), tc.data_ptr(), tf.data_ptr(), g, P, B, None) == 0
        model_commit(pool, counts, fresh, P)
        RP.sync(dev)
        assert np.array_equal(tp.cpu().numpy(), pool) and np.array_equal(u64(tc), counts), f"{what}: the commit"
        assert not tf.any()
        ctr += c
    tally.assert_presence()
    assert int(status.item()) == 0 and int(si[pkg._native.ST_STEPS].item()) == B * sum(cuts)
    ST.assert_tables_unwritten(dev, S_, "lr = 0 changed a weight")


# ---------------------------------------------------------------------------------------------------------------
# 6. racing lanes, by properties
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_racing_lanes_at_65536_boards_properties(pkg, dev):
    """65,536 lanes learning into shared tables through the agent (carousel = 512, tiles (8, 16), epsilon 0.5), 48 steps
    in launches of 8 + 40 from a reset.  Between learner and commit -- the two entry points called as the agent calls
    them -- the non-empty records of `fresh` are counted per stage: the counts grow by exactly that.  Every valid pool
    record's stage equals its row, its bytes 24..31 are zero; the statistics count every step; the weights stay finite."""
    B, P, tiles, thr, seed = 65536, 512, (8, 16), (3, 4), 31
    env = pkg.BatchedGame2048Env(B, seed=seed, device=dev)
    agent = pkg.BatchedNTupleAgent(100, learning_rate=0.05, discount_factor=0.9, exploration_rate=0.5, seed=seed,
                                   device=dev, stage_tiles=tiles, carousel=P)
    L, g = lib(pkg, dev), spec(*thr)
    agent.carousel_fresh = torch.zeros((3, B, 32), dtype=torch.uint8, device=dev)
    reported = np.zeros(3, np.int64)
    for steps in (8, 40):
        pool_before = agent.carousel_pool.clone()
        assert L.q2048_car_fused_rollout(
            env.boards.data_ptr(), env.aux.data_ptr(), agent.weights.data_ptr(), g, agent.carousel_pool.data_ptr(),
            agent.carousel_counts.data_ptr(), agent.carousel_fresh.data_ptr(), P, B, steps, 0.5, 0.05, 0.9, seed, 0,
            agent.ctr, agent.stats_i.data_ptr(), agent.stats_f.data_ptr(), agent.status.data_ptr(), None) == 0
        agent.ctr += steps
        env.ctr += steps
        RP.sync(dev)
        assert torch.equal(agent.carousel_pool, pool_before), "the learner wrote the pool"
        fresh = agent.carousel_fresh.cpu().numpy()
        has = fresh[:, :, :16].any(axis=2)
        assert not has[0].any() and not fresh[:, :, 24:].any()
        for k in (1, 2):
            assert (model_stage(fresh[k][has[k], :16], thr) == k).all(), "a record in another stage's row"
        reported += has.sum(axis=1)
        assert L.q2048_car_commit(agent.carousel_pool.data_ptr(), agent.carousel_counts.data_ptr(),
                                  agent.carousel_fresh.data_ptr(), g, P, B, None) == 0
        RP.sync(dev)
        assert not agent.carousel_fresh.any()
        assert agent.carousel_summary()["counts"] == reported.tolist()
    assert reported[1] > P and reported[2] > P, reported                     # both rings wrapped
    pool = agent.carousel_pool.cpu().numpy()
    assert not pool[0].any() and not pool[:, :, 24:].any()
    for k in (1, 2):
        assert (model_stage(pool[k, :, :16], thr) == k).all(), f"row {k} holds a board of another stage"
        assert pool[k, :, :16].any(axis=1).all()
    st = agent.stats()
    assert st["steps"] == B * 48 and 0 < st["valid_moves"] <= st["steps"] and 0 < st["explored"] <= st["valid_moves"]
    assert agent.check_status() == 0
    for k in range(3):
        assert bool(torch.isfinite(agent.weights[k]).all()), f"stage {k} holds a value that is not finite"
    assert bool((agent.weights[0] != 0).any()) and bool((agent.weights[1] != 0).any())
