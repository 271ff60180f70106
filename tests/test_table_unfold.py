"""Unfolding a symmetry-folded Q-table into a plain one: q2048_table_unfold, BatchedQLearningAgent.unfold_from,
export_dict(unfold=True), merge_tables.py --unfold, train.py --resume FOLDED --unfold.

The checking model is independent numpy, written from include/q2048.h: a key is unpacked into a 4x4 array, its images
are np.rot90 / np.fliplr, the canonical image is the smallest packed key (the smallest g on a tie), the action
permutation is the header's table copied by hand, and every float32 product and sum is a numpy operation of its own.
It never calls q2048_canonicalize.  Rows are compared AS BIT PATTERNS ({key: 16 value bytes}), no tolerance anywhere.
Every test runs on the CPU twin ("cpu") and on the GPU."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
DEVICES = ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)]
MODES = [("add", 1.0), ("add", 0.25), ("blend", 0.3), ("blend", 0.0), ("blend", 1.0), ("maxabs", 1.0)]
MERGE_ID = {"add": 0, "blend": 1, "maxabs": 2}
# pi_g(a), include/q2048.h (Q2048_FLAG_SYMMETRIC), row g, column a -- copied from the header's table
PI = [[0, 1, 2, 3], [3, 0, 1, 2], [2, 3, 0, 1], [1, 2, 3, 0], [2, 1, 0, 3], [1, 0, 3, 2], [0, 3, 2, 1], [3, 2, 1, 0]]
F32 = np.float32
TABLE_FULL, DEEP_ROW = 4, 8


def sync(dev):
    if str(dev) != "cpu":
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
def unpack(key):
    """key -> the [4][4] array of log2 cells (cell 4r + c in nibble 4r + c)."""
    return np.array([(int(key) >> (4 * i)) & 15 for i in range(16)], dtype=np.uint8).reshape(4, 4)


def pack(b):
    return sum(int(v) << (4 * i) for i, v in enumerate(np.asarray(b).reshape(-1)))


def images(b):
    """g = 0..3: np.rot90(b, g); g = 4..7: np.rot90(np.fliplr(b), g - 4)."""
    return [np.rot90(b, g) for g in range(4)] + [np.rot90(np.fliplr(b), g) for g in range(4)]


@functools.lru_cache(maxsize=None)
def canon(key):
    """(canonical key, g): the smallest image key, on a tie the smallest g."""
    ks = [pack(x) for x in images(unpack(key))]
    c = min(ks)
    return c, ks.index(c)


@functools.lru_cache(maxsize=None)
def members(c):
    """image_h(c), h = 0..7 in ascending h, an h whose key equals that of a smaller h left out."""
    out = []
    for x in images(unpack(c)):
        k = pack(x)
        if k not in out:
            out.append(k)
    return tuple(out)


def member_row(m, qc):
    """The row of member m in its own frame: Q_m[a] = Qc[pi_g(a)], g = the smallest g with image_g(m) = c."""
    g = canon(m)[1]
    return np.array([qc[PI[g][a]] for a in range(4)], F32)


def combine(out, dst, key, r, mode, w32, keep):
    """The merge's formulas for one source row r that meets dst: returns "created" or "combined"."""
    with np.errstate(all="ignore"):
        if key not in dst:
            out[key] = (w32 * r).astype(F32) if mode == "add" else r.copy()
            return "created"
        d = dst[key]
        if mode == "add":
            ws = (w32 * r).astype(F32)
            out[key] = (d + ws).astype(F32)
        elif mode == "blend":
            a, b = (keep * d).astype(F32), (w32 * r).astype(F32)
            out[key] = (a + b).astype(F32)
        else:
            out[key] = np.where(np.abs(r) > np.abs(d), r, d).astype(F32)
        return "combined"


def model_unfold(dst, src, mode, w):
    """dst, src: {key: float32[4]}.  Returns (rows after, counters[6]) -- with room for every member ([5] = 0)."""
    w32 = F32(w)
    keep = F32(F32(1.0) - w32)                           # 1 - w, once, in float32
    out, n = dict(dst), {"created": 0, "combined": 0}
    read = skipped = 0
    for c in sorted(src):
        read += 1
        if canon(c)[0] != c:
            skipped += 1
            continue
        for m in members(c):
            n[combine(out, dst, m, member_row(m, src[c]), mode, w32, keep)] += 1
    return out, [read, skipped, n["created"] + n["combined"], n["created"], n["combined"], 0]


def model_merge(dst, src, mode, w):
    w32 = F32(w)
    keep = F32(F32(1.0) - w32)
    out = dict(dst)
    for k in src:
        combine(out, dst, k, src[k], mode, w32, keep)
    return out


def as_dict(rows):
    keys, q = rows
    d = {int(k): np.array(v, F32) for k, v in zip(np.asarray(keys).reshape(-1).tolist(), q)}
    assert len(d) == len(q), "a key occurs twice in the export"
    return d


def as_rows(d):
    keys = np.array(sorted(d), dtype=np.uint64)
    return keys, np.stack([d[int(k)] for k in keys]).astype(F32) if len(keys) else np.zeros((0, 4), F32)


def assert_same(got, want, what=""):
    assert sorted(got) == sorted(want), f"{what}: key sets differ ({len(got)} rows, the model has {len(want)})"
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), \
            f"{what}: key {k:#018x}: {got[k]} ({got[k].view(np.uint32)}), the model has {want[k]} ({want[k].view(np.uint32)})"


# ---------------------------------------------------------------------------------------------
# agents and hand-built sources
# ---------------------------------------------------------------------------------------------
def new_agent(pkg, dev, cap, symmetric, **kw):
    kw.setdefault("freeze_load", None)
    kw.setdefault("placement", "plain")
    return pkg.BatchedQLearningAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.3, capacity_log2=cap,
                                     seed=1, env_id0=0, device=dev, board_size=4, symmetric=symmetric, **kw)


def agent_with(pkg, dev, cap, symmetric, d):
    agent = new_agent(pkg, dev, cap, symmetric)
    if d:
        agent.import_rows(*as_rows(d))
    return agent


def generic_board(rng):
    """A board with eight distinct images, as its canonical key."""
    while True:
        c = canon(pack(rng.integers(0, 12, size=(4, 4))))[0]
        if len(members(c)) == 8 and c != 0:
            return c


MIRROR = [[1, 2, 2, 1], [3, 4, 4, 3], [5, 6, 6, 5], [7, 8, 8, 7]]           # equal to its own np.fliplr: 4 images
DIAGONAL = [[1, 2, 3, 4], [2, 5, 6, 7], [3, 6, 8, 9], [4, 7, 9, 10]]        # equal to its transpose: 4 images
MIRROR_BOTH = [[1, 2, 2, 1], [3, 4, 4, 3], [3, 4, 4, 3], [1, 2, 2, 1]]      # ... fliplr and flipud: 2 images
DIAGONALS = [[1, 2, 3, 4], [2, 5, 6, 3], [3, 6, 5, 2], [4, 3, 2, 1]]        # transpose and anti-transpose: 2 images
HALF_TURN_4 = [[1, 2, 3, 4], [5, 6, 7, 8], [8, 7, 6, 5], [4, 3, 2, 1]]      # equal to its half turn only: 4 images
ALL_EQUAL = [[3] * 4] * 4                                                   # 1 image
ALL_SYMMETRIC = [[1, 2, 2, 1], [2, 3, 3, 2], [2, 3, 3, 2], [1, 2, 2, 1]]    # equal to transpose and mirror: 1 image


def values(rng, k):
    """k rows: random float32 of both signs, exact +0.0 and -0.0 entries."""
    v = (rng.standard_normal((k, 4)) * 10.0).astype(F32)
    zero = rng.random((k, 4))
    v[zero < 0.2] = F32(0.0)
    v[(zero >= 0.2) & (zero < 0.3)] = F32(-0.0)
    return v


_HAND = {}


def hand_built(seed=7):
    """The folded source of most tests (built once): {canonical key: row}, at least 4 orbits of each shape -- 8, 4, 2
    and 1 distinct images -- the symmetric boards built explicitly and their image counts asserted."""
    if seed not in _HAND:
        rng = np.random.default_rng(seed)
        keys = {8: [generic_board(rng) for _ in range(12)], 4: [], 2: [], 1: []}
        for board, count, shifts in ((MIRROR, 4, 2), (DIAGONAL, 4, 2), (HALF_TURN_4, 4, 2), (MIRROR_BOTH, 2, 3),
                                     (DIAGONALS, 2, 3), (ALL_EQUAL, 1, 3), (ALL_SYMMETRIC, 1, 3)):
            for shift in range(shifts):
                c = canon(pack(np.array(board) + shift))[0]
                assert len(members(c)) == count, (board, shift)
                keys[count].append(c)
        flat = [c for cs in keys.values() for c in cs]
        assert len(set(flat)) == len(flat) and all(len(cs) >= 4 for cs in keys.values())
        assert {len(members(c)) for c in flat} == {8, 4, 2, 1}
        vals = values(rng, len(flat))
        src = {c: vals[i] for i, c in enumerate(flat)}
        bits = np.stack(list(src.values())).view(np.uint32)
        assert (bits == 0).any() and (bits == 0x80000000).any() and (np.stack(list(src.values())) < 0).any()
        _HAND[seed] = src
    return _HAND[seed]


def generic_keys(seed, count):
    """`count` distinct canonical keys of stabiliser-free boards, vectorised (numpy only): uint64[count]."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 12, size=(count + count // 8 + 64, 4, 4)).astype(np.uint64)
    imgs = [np.rot90(b, g, axes=(1, 2)) for g in range(4)] + [np.rot90(b[:, :, ::-1], g, axes=(1, 2)) for g in range(4)]
    shifts = (np.arange(16, dtype=np.uint64) * np.uint64(4)).reshape(1, 16)
    ks = np.stack([(x.reshape(-1, 16) << shifts).sum(axis=1, dtype=np.uint64) for x in imgs], axis=1)   # [N, 8]
    free = np.array([len(set(row)) == 8 for row in ks.tolist()])
    c = np.unique(ks[free].min(axis=1))
    c = c[c != 0]
    assert len(c) >= count
    return rng.permutation(c)[:count]


def same_stats(a, b):
    """Two statistics dicts are equal, a mean over no episode (nan) being equal to itself."""
    return a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def check_unfold(pkg, dst, src, mode, w, what=""):
    """unfold_from against the model, with the identities the counters and the bookkeeping owe."""
    before, other = as_dict(dst.export_rows()), as_dict(src.export_rows())
    src_table = src.table.clone()
    out = dst.unfold_from(src, mode=mode, weight=w)
    sync(dst.device)
    want, ctr = model_unfold(before, other, mode, w)
    got = [out[k] for k in ("read", "skipped", "written", "created", "combined", "dropped")]
    assert got == ctr, (what, out, ctr)
    assert out["written"] == out["created"] + out["combined"] + out["dropped"]
    assert out["written"] == sum(len(members(c)) for c in other)
    assert dst.table_size() == len(before) + out["created"]
    dst.stats(verify=True)
    assert torch.equal(src.table, src_table), "the source was written"
    assert_same(as_dict(dst.export_rows()), want, what)
    return out, want


# ---------------------------------------------------------------------------------------------
# 1. symbol and signature
# ---------------------------------------------------------------------------------------------
def test_both_libraries_export_the_unfold(pkg):
    N = pkg._native
    assert "q2048_table_unfold" in N._SIGNATURES
    res, args = N._SIGNATURES["q2048_table_unfold"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
    assert hasattr(C.CDLL(N.HOST_LIB_PATH), "q2048_table_unfold")
    assert hasattr(C.CDLL(N.LIB_PATH), "q2048_table_unfold")         # loads without a GPU: no compute call here
    assert N.host_lib().q2048_abi_version() == N.lib().q2048_abi_version() == 7   # additive: detected by its symbol
    with open(os.path.join(REPO, "include", "q2048.h")) as fh:
        assert "int q2048_table_unfold(q2048_slot *dst, int dst_cap_log2, const q2048_slot *src, int src_cap_log2" in fh.read()
    for g in range(8):                                               # the model's permutation table is the header's formula
        for a in range(4):
            assert PI[g][a] == ((a - g) & 3 if g < 4 else (2 - a - (g - 4)) & 3)


# ---------------------------------------------------------------------------------------------
# 2. hand-built orbits, every mode, empty and prefilled destinations
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("mode,w", MODES)
def test_hand_built_orbits_equal_the_model(pkg, dev, mode, w):
    rows = hand_built()
    src = agent_with(pkg, dev, 8, True, rows)
    out, want = check_unfold(pkg, new_agent(pkg, dev, 10, False), src, mode, w, f"empty, {mode} w={w}")
    assert out["read"] == len(rows) and out["skipped"] == out["combined"] == out["dropped"] == 0
    assert out["created"] == len(want) == sum(len(members(c)) for c in rows)

    # a destination that holds some members of some orbits, none of others, and unrelated keys
    rng = np.random.default_rng(11)
    held = {}
    for i, c in enumerate(sorted(rows)):
        ms = members(c)
        if i % 3 == 0:
            pick = ms                                                 # every member
        elif i % 3 == 1:
            pick = ms[1::2] if len(ms) > 1 else ms                    # some, the canonical one not among them
        else:
            pick = ()
        for m in pick:
            held[m] = values(rng, 1)[0]
    others = {}
    while len(others) < 30:
        c = generic_board(rng)
        if c not in rows:
            others[members(c)[int(rng.integers(8))]] = values(rng, 1)[0]
    dst = agent_with(pkg, dev, 10, False, {**held, **others})
    out, _ = check_unfold(pkg, dst, src, mode, w, f"prefilled, {mode} w={w}")
    assert out["combined"] == len(held) > 0 and out["created"] == len(want) - len(held) > 0
    after = as_dict(dst.export_rows())
    for k, r in others.items():
        assert after[k].tobytes() == r.tobytes()


# ---------------------------------------------------------------------------------------------
# 3. the frame's direction, as literals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_frame_direction(pkg, dev):
    c = generic_board(np.random.default_rng(3))
    b = unpack(c)
    src = agent_with(pkg, dev, 8, True, {c: np.array([10.0, 20.0, 30.0, 40.0], F32)})
    dst = new_agent(pkg, dev, 8, False)
    out = dst.unfold_from(src)
    assert out == {"read": 1, "skipped": 0, "written": 8, "created": 8, "combined": 0, "dropped": 0}
    got = as_dict(dst.export_rows())
    quarter, mirror = pack(np.rot90(b, 1)), pack(np.fliplr(b))
    assert pack(np.rot90(np.rot90(b, 1), 3)) == c                    # the quarter turn's own g is 3, pi_3 = 1 2 3 0
    assert got[quarter].tolist() == [20.0, 30.0, 40.0, 10.0]
    assert got[mirror].tolist() == [30.0, 20.0, 10.0, 40.0]
    assert got[c].tolist() == [10.0, 20.0, 30.0, 40.0]


# ---------------------------------------------------------------------------------------------
# 4. the unfolded table reads as the folded one does; 5. the round trip; 10. export_dict(unfold=True)
# ---------------------------------------------------------------------------------------------
_TRAINED = {}


def trained_pair(pkg, dev):
    """A symmetric agent trained by fused_rollout (64 envs x 200 steps, seed 1, 2^14 slots), its final boards, and
    the plain agent it unfolds into -- made once per device and left unchanged by the tests that read it."""
    if dev not in _TRAINED:
        env = pkg.BatchedGame2048Env(64, board_size=4, seed=1, env_id0=0, device=dev)
        folded = new_agent(pkg, dev, 14, True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                           # (a fixed table past load 0.35 says so)
            for _ in range(4):
                folded.fused_rollout(env, 50)
        sync(dev)
        assert folded.check_status() == 0
        rows = folded.table_size()
        plain = new_agent(pkg, dev, max(10, int(np.ceil(np.log2(16.0 * rows)))), False)
        table = folded.table.clone()
        out = plain.unfold_from(folded)
        sync(dev)
        assert out["read"] == rows and out["skipped"] == out["dropped"] == out["combined"] == 0
        assert 4 * rows < out["created"] == out["written"] == plain.table_size() <= 8 * rows
        plain.stats(verify=True)
        assert torch.equal(folded.table, table)
        _TRAINED[dev] = (folded, plain, env.boards.cpu().numpy().copy())
    return _TRAINED[dev]


@pytest.mark.parametrize("dev", DEVICES)
def test_unfolded_table_answers_q_values_as_the_folded_one(pkg, dev):
    folded, plain, final = trained_pair(pkg, dev)
    batch = np.stack([np.ascontiguousarray(x).reshape(16) for b in final for x in images(b.reshape(4, 4))])
    assert {canon(pack(b))[1] for b in batch} == set(range(8))
    boards = torch.from_numpy(batch).to(dev)
    qf, ff = folded.q_values(boards, return_found=True)
    qp, fp = plain.q_values(boards, return_found=True)
    sync(dev)
    assert torch.equal(ff, fp) and bool(ff.any())
    assert torch.equal(qf.view(torch.int32), qp.view(torch.int32))
    assert bool((qf != 0).any())


@pytest.mark.parametrize("dev", DEVICES)
def test_unfolded_table_plays_and_evaluates_as_the_folded_one(pkg, dev):
    folded, plain, _ = trained_pair(pkg, dev)
    tables = [folded.table.clone(), plain.table.clone()]
    reads_a_row = False
    for id0 in (0, 1000):                                             # two fresh batches of the training seed
        for eps in (0.0, 0.25):
            ends = []
            for agent in (folded, plain):
                env = pkg.BatchedGame2048Env(64, board_size=4, seed=1, env_id0=id0, device=dev)
                reads_a_row |= bool((agent.q_values(env.boards) != 0).any())
                agent.play_stats(reset=True)
                agent.play_rollout(env, 300, epsilon=eps)
                sync(dev)
                ends.append((env.boards.clone(), env.aux.clone(), agent.play_stats(reset=True)))
            assert torch.equal(ends[0][0], ends[1][0]) and torch.equal(ends[0][1], ends[1][1]), (id0, eps)
            assert same_stats(ends[0][2], ends[1][2]) and ends[0][2]["steps"] == 64 * 300, (id0, eps)
    assert reads_a_row                                                # the table matters
    # evaluation: the fused rollout that only reads
    ends = []
    for agent in (folded, plain):
        env = pkg.BatchedGame2048Env(64, board_size=4, seed=1, env_id0=0, device=dev)
        ctr, eps = agent.ctr, agent.epsilon
        agent.ctr, agent.epsilon = env.ctr, 0.1                       # (one draw stream, one epsilon for both)
        agent.stats(reset=True)
        agent.fused_rollout(env, 300, learn=False)
        sync(dev)
        assert agent.check_status() == 0
        ends.append((env.boards.clone(), env.aux.clone(), agent.stats()))
        agent.ctr, agent.epsilon = ctr, eps
    assert torch.equal(ends[0][0], ends[1][0]) and torch.equal(ends[0][1], ends[1][1])
    assert same_stats(ends[0][2], ends[1][2]) and ends[0][2]["steps"] == 64 * 300 and ends[0][2]["inserts"] == 0
    assert torch.equal(folded.table, tables[0]) and torch.equal(plain.table, tables[1])


@pytest.mark.parametrize("dev", DEVICES)
def test_round_trip(pkg, dev):
    """fold_from(unfolded, fold="maxabs") gives the folded rows back: every member carries the orbit's row, and the
    entry of larger magnitude among equal entries is that entry."""
    hand = agent_with(pkg, dev, 8, True, hand_built())
    hand_plain = new_agent(pkg, dev, 10, False)
    hand_plain.unfold_from(hand)
    for folded, plain in (trained_pair(pkg, dev)[:2], (hand, hand_plain)):
        back = new_agent(pkg, dev, plain.capacity_log2, True)
        out = back.fold_from(plain, fold="maxabs")
        sync(dev)
        assert out["orbits"] == out["created"] == folded.table_size() and out["read"] == plain.table_size()
        assert_same(as_dict(back.export_rows()), as_dict(folded.export_rows()), "round trip")


@pytest.mark.parametrize("dev", DEVICES)
def test_export_dict_unfold(pkg, dev):
    folded = agent_with(pkg, dev, 8, True, hand_built())
    table = folded.table.clone()
    canonical = folded.export_dict()
    full = folded.export_dict(unfold=True)
    assert torch.equal(folded.table, table)
    raw = lambda key: tuple(tuple(0 if v == 0 else 1 << int(v) for v in row) for row in unpack(key))   # noqa: E731
    assert set(canonical) == {raw(c) for c in hand_built()}                        # export_dict() is what it was
    for c, r in hand_built().items():
        assert canonical[raw(c)].dtype == np.float64 and canonical[raw(c)].tolist() == r.astype(np.float64).tolist()
    assert folded.export_dict(unfold=False).keys() == canonical.keys()
    want_keys = [m for c in hand_built() for m in members(c)]
    assert set(full) == {raw(m) for m in want_keys} and len(full) == len(want_keys) > len(canonical)
    boards = torch.from_numpy(np.stack([unpack(m).reshape(16) for m in want_keys])).to(dev)
    q = folded.q_values(boards).cpu().numpy().astype(np.float64)
    for m, row in zip(want_keys, q):
        assert full[raw(m)].dtype == np.float64 and full[raw(m)].tobytes() == row.tobytes()
    plain = agent_with(pkg, dev, 8, False, hand_built())
    a, b = plain.export_dict(), plain.export_dict(unfold=True)
    assert a.keys() == b.keys() == canonical.keys() and all(a[k].tobytes() == b[k].tobytes() for k in a)


# ---------------------------------------------------------------------------------------------
# 6. the raw call through ctypes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_through_ctypes(pkg, dev):
    """Counters are added to; `src` keeps every byte, line summaries in its spare words included, and the result is
    the same with them; the `reserved` words of `dst` stay what they were; non-canonical keys in `src` are counted and
    leave no trace; status == NULL is accepted."""
    N = pkg._native
    rows = dict(hand_built())
    rng = np.random.default_rng(5)
    stray = {}
    while len(stray) < 5:                                             # keys a folded table never holds
        c = generic_board(rng)
        if c not in rows:
            stray[members(c)[1 + len(stray)]] = values(rng, 1)[0]
    assert all(canon(k)[0] != k for k in stray)
    src = agent_with(pkg, dev, 8, True, {**rows, **stray})
    want, ctr = model_unfold({}, {**rows, **stray}, "blend", 0.3)
    assert ctr[1] == 5 and ctr[0] == len(rows) + 5
    assert not any(m in want for k in stray for m in members(canon(k)[0]))
    results = []
    for summaries in (False, True):
        if summaries:
            N.check(src._L.q2048_table_summarise(src.table.data_ptr(), 8, None), "table_summarise")
            sync(dev)
            assert bool((src.table.view(torch.int64).reshape(-1, 4)[:, 3] != 0).any())
        before = src.table.clone()
        dst = new_agent(pkg, dev, 10, False)
        marks = torch.arange(1, (1 << 10) + 1, dtype=torch.int64, device=dev) * 0x0101
        dst.table.view(torch.int64).reshape(-1, 4)[:, 3] = marks     # the spare words of dst: every one its own mark
        counters = torch.tensor([6, 5, 4, 3, 2, 1], dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        N.check(dst._L.q2048_table_unfold(dst.table.data_ptr(), 10, src.table.data_ptr(), 8, 1, MERGE_ID["blend"], 0.3,
                                          counters.data_ptr(), status.data_ptr() if summaries else None, None),
                "table_unfold")
        sync(dev)
        assert torch.equal(src.table, before)
        assert counters.tolist() == [6 + ctr[0], 5 + ctr[1], 4 + ctr[2], 3 + ctr[3], 2 + ctr[4], 1] and int(status.item()) == 0
        assert torch.equal(dst.table.view(torch.int64).reshape(-1, 4)[:, 3], marks)
        dst.recount_rows()
        got = as_dict(dst.export_rows())
        assert_same(got, want, "raw call")
        results.append(got)
    assert_same(results[0], results[1], "with and without summaries in src")
    # 5x5 tables are refused before anything is touched
    code = dst._L.q2048_table_unfold(dst.table.data_ptr(), 10, src.table.data_ptr(), 8, 2, 0, 1.0, counters.data_ptr(),
                                     status.data_ptr(), None)
    assert code == -4                                                                # Q2048_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------
# 7. probe and stride edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_source_larger_than_one_grid_pass(pkg, dev):
    """The launch caps its grid at 2048 blocks of 256 lanes: a 2^20-slot source takes two passes of the grid-stride
    loop."""
    rows = hand_built()
    src = agent_with(pkg, dev, 20, True, rows)
    slots = torch.nonzero(src.table.view(torch.int64).reshape(-1, 4)[:, 0] != 0).reshape(-1)
    assert int((slots >= (1 << 19)).sum()) > 5 and int((slots < (1 << 19)).sum()) > 5
    check_unfold(pkg, new_agent(pkg, dev, 10, False), src, "add", 0.25, "2^20-slot source")


@pytest.mark.parametrize("dev", DEVICES)
def test_small_source_at_load_080(pkg, dev):
    """2^8 slots, 205 rows: the stream meets long runs of occupied slots."""
    keys = [int(k) for k in generic_keys(21, 205 - len(hand_built()))]
    vals = values(np.random.default_rng(22), len(keys))
    rows = {**hand_built(), **{k: vals[i] for i, k in enumerate(keys)}}
    assert len(rows) == 205
    src = agent_with(pkg, dev, 8, True, rows)
    assert src.capacity_log2 == 8 and src.table_size() == 205
    check_unfold(pkg, new_agent(pkg, dev, 12, False), src, "blend", 0.3, "load 0.8")


@pytest.mark.parametrize("dev", DEVICES)
def test_destination_at_load_085_equals_a_roomy_one(pkg, dev):
    keys = [int(k) for k in generic_keys(31, 27)]
    two = next(c for c in hand_built() if len(members(c)) == 2)
    vals = values(np.random.default_rng(32), 28)
    rows = {k: vals[i] for i, k in enumerate(keys + [two])}
    src = agent_with(pkg, dev, 8, True, rows)
    tight, roomy = new_agent(pkg, dev, 8, False), new_agent(pkg, dev, 12, False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                # (no deep row: the probe limit is the table)
        check_unfold(pkg, tight, src, "add", 0.25, "load 0.85")
        check_unfold(pkg, roomy, src, "add", 0.25, "roomy")
    assert tight.table_size() == 218 and tight.capacity_log2 == 8    # 218 / 256 = 0.85
    assert_same(as_dict(tight.export_rows()), as_dict(roomy.export_rows()), "tight against roomy")


@pytest.mark.parametrize("dev", DEVICES)
def test_destination_too_small(pkg, dev):
    """A 16-slot destination for 4 orbits of 8: TABLE_FULL, 16 members dropped, every row that is there is right."""
    N = pkg._native
    keys = [int(k) for k in generic_keys(41, 4)]
    vals = values(np.random.default_rng(42), 4)
    rows = {k: vals[i] for i, k in enumerate(keys)}
    src = agent_with(pkg, dev, 8, True, rows)
    dst = new_agent(pkg, dev, 4, False)
    counters = torch.zeros(6, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    N.check(dst._L.q2048_table_unfold(dst.table.data_ptr(), 4, src.table.data_ptr(), 8, 1, MERGE_ID["add"], 1.0,
                                      counters.data_ptr(), status.data_ptr(), None), "table_unfold")
    sync(dev)
    want, _ = model_unfold({}, rows, "add", 1.0)
    assert len(want) == 32
    assert int(status.item()) & TABLE_FULL
    assert counters.tolist() == [4, 0, 32, 16, 0, 16]
    assert dst.recount_rows() == 16 == len(want) - int(counters[5])
    got = as_dict(dst.export_rows())
    assert set(got) <= set(want)
    for k, r in got.items():
        assert r.tobytes() == want[k].tobytes()


# ---------------------------------------------------------------------------------------------
# 8. argument errors in order
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hip", "host"])
def test_abi_argument_errors(pkg, which):
    """One call per error, fake aligned addresses otherwise: validation runs on the host before anything is launched
    (or, on the CPU twin, touched)."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    f = L.q2048_table_unfold
    d, s, c, st = 1 << 30, 1 << 40, 1 << 20, 1 << 21
    NULL, SIZE, ALIGN, UNSUPPORTED, RANGE, FLAGS = -1, -2, -3, -4, -6, -7
    assert f(None, 20, s, 20, 1, 0, 1.0, c, st, None) == NULL
    assert f(d, 20, None, 20, 1, 0, 1.0, c, st, None) == NULL
    assert f(d, 20, s, 20, 1, 0, 1.0, None, st, None) == NULL
    assert f(d, 20, s, 20, 2, 0, 1.0, c, st, None) == UNSUPPORTED          # 5x5
    assert f(d, 20, s, 20, 0, 0, 1.0, c, st, None) == SIZE
    assert f(d, 20, s, 20, 3, 0, 1.0, c, st, None) == SIZE
    assert f(d, 3, s, 20, 1, 0, 1.0, c, st, None) == SIZE
    assert f(d, 41, s, 20, 1, 0, 1.0, c, st, None) == SIZE
    assert f(d, 20, s, 3, 1, 0, 1.0, c, st, None) == SIZE
    assert f(d, 20, s, 41, 1, 0, 1.0, c, st, None) == SIZE
    assert f(d + 8, 20, s, 20, 1, 0, 1.0, c, st, None) == ALIGN
    assert f(d, 20, s + 8, 20, 1, 0, 1.0, c, st, None) == ALIGN
    assert f(d, 20, s, 20, 1, 3, 1.0, c, st, None) == FLAGS
    assert f(d, 20, s, 20, 1, -1, 1.0, c, st, None) == FLAGS
    assert f(d, 20, s, 20, 1, 0, float("nan"), c, st, None) == RANGE
    assert f(d, 20, s, 20, 1, 2, float("inf"), c, st, None) == RANGE
    assert f(d, 20, s, 20, 1, 1, 1.5, c, st, None) == RANGE
    assert f(d, 20, s, 20, 1, 1, -0.25, c, st, None) == RANGE
    assert f(d, 20, d, 20, 1, 0, 1.0, c, st, None) == RANGE                       # src == dst
    assert f(d, 20, d + (32 << 20) - 32, 20, 1, 0, 1.0, c, st, None) == RANGE     # the last slot of dst is src's first
    assert f(d + (32 << 16) - 32, 20, d, 16, 1, 0, 1.0, c, st, None) == RANGE     # ... and the other way round
    # the order: NULL, UNSUPPORTED, SIZE, ALIGN, FLAGS, RANGE (w), RANGE (overlap)
    assert f(None, 99, s + 8, 20, 2, 9, float("nan"), c, st, None) == NULL
    assert f(d + 8, 99, s, 20, 2, 9, float("nan"), c, st, None) == UNSUPPORTED
    assert f(d + 8, 99, s, 20, 1, 9, float("nan"), c, st, None) == SIZE
    assert f(d + 8, 20, s, 20, 1, 9, float("nan"), c, st, None) == ALIGN
    assert f(d, 20, s, 20, 1, 9, float("nan"), c, st, None) == FLAGS
    assert f(d, 20, d, 20, 1, 0, float("nan"), c, st, None) == RANGE
    assert f(d, 20, d, 20, 1, 1, 0.5, c, st, None) == RANGE


# ---------------------------------------------------------------------------------------------
# 9. the agent's refusals and its sizing
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_agent_refusals_and_sizing(pkg, dev):
    plain, other_plain = new_agent(pkg, dev, 8, False), new_agent(pkg, dev, 8, False)
    folded, other_folded = new_agent(pkg, dev, 8, True), new_agent(pkg, dev, 8, True)
    with pytest.raises(ValueError, match="merge_from combines two folded tables"):
        folded.unfold_from(other_folded)
    with pytest.raises(ValueError, match="merge_from combines"):
        plain.unfold_from(other_plain)
    with pytest.raises(ValueError):
        plain.unfold_from(plain)
    with pytest.raises(ValueError):
        plain.unfold_from("a table")
    five = pkg.BatchedQLearningAgent(10, capacity_log2=8, device=dev, board_size=5, placement="plain", freeze_load=None)
    with pytest.raises(ValueError, match="board size 4"):
        five.unfold_from(folded)
    with pytest.raises(ValueError, match="independent"):
        new_agent(pkg, dev, 8, False, independent=True).unfold_from(folded)
    with pytest.raises(ValueError, match="independent"):
        plain.unfold_from(new_agent(pkg, dev, 8, True, independent=True))
    with pytest.raises(ValueError, match="mode"):
        plain.unfold_from(folded, mode="mean")
    with pytest.raises(ValueError, match="weight"):
        plain.unfold_from(folded, mode="blend", weight=1.5)
    with pytest.raises(ValueError, match="weight"):
        plain.unfold_from(folded, weight=float("nan"))
    if dev != "cpu":
        with pytest.raises(ValueError, match="different devices"):
            plain.unfold_from(new_agent(pkg, "cpu", 8, True))
    # the mix stays refused where no unfold was asked for
    with pytest.raises(ValueError, match="folded"):
        plain.merge_from(folded)
    with pytest.raises(ValueError, match="folded"):
        plain.load_state_dict(folded.state_dict())
    # a destination whose key set is closed refuses
    env = pkg.BatchedGame2048Env(512, board_size=4, seed=1, env_id0=0, device=dev)
    frozen = new_agent(pkg, dev, 10, False, freeze_load=0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(6):
            frozen.fused_rollout(env, 20)
    sync(dev)
    assert frozen.frozen
    with pytest.raises(ValueError, match="closed"):
        frozen.unfold_from(folded)
    # a fixed table too small for 8x the source's rows: refused before anything is launched
    src = agent_with(pkg, dev, 8, True, hand_built())                 # 30 rows: the bound is 240 > 0.9 * 256
    assert 8 * len(hand_built()) > 0.9 * 256 > sum(len(members(c)) for c in hand_built())
    tiny = agent_with(pkg, dev, 8, False, {members(c)[-1]: r for c, r in list(hand_built().items())[:3]})
    before = tiny.table.clone()
    with pytest.raises(ValueError, match="too small"):
        tiny.unfold_from(src)
    assert torch.equal(tiny.table, before) and tiny.table_size() == 3
    # a table that can grow grows first, until 8x the source's rows (and its own) fit half of it
    keys = generic_keys(51, 5000)
    vals = values(np.random.default_rng(52), 5000)
    big = new_agent(pkg, dev, 14, True)
    big.import_rows(keys, vals)
    dst = new_agent(pkg, dev, "auto", False, initial_capacity_log2=16, max_capacity_log2=22, prefetch_growth=False)
    assert dst.growable and dst.capacity_log2 == 16 and not dst.growths
    out = dst.unfold_from(big, mode="blend", weight=1.0)
    sync(dev)
    assert out == {"read": 5000, "skipped": 0, "written": 40000, "created": 40000, "combined": 0, "dropped": 0}
    assert dst.growths and dst.growths[-1]["to_log2"] == dst.capacity_log2 == 17
    assert dst.stats(verify=True) is not None and dst.table_size() == 40000
    assert dst.verify_table()["rows"] == 40000


# ---------------------------------------------------------------------------------------------
# 11. the scripts
# ---------------------------------------------------------------------------------------------
def test_scripts_unfold(pkg, tmp_path):
    py = lambda script, *a: subprocess.run([sys.executable, os.path.join(REPO, script), "--device", "cpu", *a],   # noqa: E731
                                           capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    small = ("--num-envs", "64", "--steps-per-launch", "16", "--max-steps", "32")
    p = py("train.py", *small, "--capacity-log2", "16", "--episodes", "2", "--symmetric", "--save", "A.pt", "--log", "a.csv")
    assert p.returncode == 0, p.stderr[-2000:]
    p = py("train.py", *small, "--capacity-log2", "16", "--episodes", "2", "--seed", "2", "--save", "P.pt", "--log", "p.csv")
    assert p.returncode == 0, p.stderr[-2000:]
    A, P = (torch.load(tmp_path / f, map_location="cpu", weights_only=False) for f in ("A.pt", "P.pt"))
    assert A["symmetric"] is True and "symmetric" not in P
    a_rows, p_rows = as_dict((A["keys"], A["q"])), as_dict((P["keys"], P["q"]))

    # merge_tables.py --unfold: one folded and one plain file -> the mean, a plain table
    p = py("merge_tables.py", "--unfold", "--mode", "mean", "--out", "M.pt", "A.pt", "P.pt")
    assert p.returncode == 0, p.stderr[-2000:]
    report = json.loads(p.stdout.strip().splitlines()[-1])
    M = torch.load(tmp_path / "M.pt", map_location="cpu", weights_only=False)
    want, ctr = model_unfold({}, a_rows, "add", 0.5)
    want = model_merge(want, p_rows, "add", 0.5)
    assert "symmetric" not in M and M["merged"]["unfolded_inputs"] == ["A.pt"] and M["merged"]["mode"] == "mean"
    assert_same(as_dict((M["keys"], M["q"])), want, "merge_tables.py --unfold")
    assert report["unfold"] is True and report["rows_out"] == len(want)
    assert [report["merges"][0][k] for k in ("read", "skipped", "written", "created", "combined", "dropped")] == ctr
    assert report["merges"][1]["read"] == len(p_rows)
    p = py("merge_tables.py", "--unfold", "--fold", "mean", "--out", "bad.pt", "A.pt", "P.pt")
    assert p.returncode != 0 and "exclude each other" in p.stderr and not (tmp_path / "bad.pt").exists()
    p = py("merge_tables.py", "--mode", "sum", "--out", "bad.pt", "A.pt", "P.pt")
    assert p.returncode != 0 and "cannot be merged" in p.stderr and not (tmp_path / "bad.pt").exists()

    # train.py --resume FOLDED --unfold --deterministic: the folded file goes on as a plain table
    resume = ("train.py", *small, "--capacity-log2", "18", "--resume", "A.pt", "--deterministic", "--episodes", "3",
              "--log", "b.csv")
    p = py(*resume, "--unfold", "--save", "B.pt")
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"unfolded A.pt: {len(a_rows)} folded rows" in p.stdout
    B = torch.load(tmp_path / "B.pt", map_location="cpu", weights_only=False)
    assert "symmetric" not in B and "visit_rows" not in B and B["train"]["epoch"] >= A["train"]["epoch"]
    assert {m for c in a_rows for m in members(c)} <= set(B["keys"].tolist())
    assert int(B["stats_i"][0]) > int(A["stats_i"][0])                               # the statistics went on
    p = py(*resume)
    assert p.returncode != 0 and "do not load into each other" in p.stderr           # the refusal of today
    p = py(*resume[:-5], "--episodes", "3", "--log", "c.csv", "--unfold", "--symmetric")   # (no --deterministic)
    assert p.returncode != 0 and "--symmetric" in p.stderr
    p = py("train.py", *small, "--episodes", "3", "--unfold", "--log", "d.csv")
    assert p.returncode != 0 and "--resume" in p.stderr
    p = py("train.py", *small, "--capacity-log2", "18", "--episodes", "3", "--seed", "2", "--resume", "P.pt", "--unfold",
           "--log", "e.csv")
    assert p.returncode != 0 and "already holds a plain table" in p.stderr


# ---------------------------------------------------------------------------------------------
# 12. many blocks, against the CPU twin (GPU only)
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_many_orbits_equal_the_cpu_twin(pkg):
    """65 536 stabiliser-free orbits -> 524 288 member rows into 2^21 slots, add with w = 0.25: many blocks, the wave and
    block reduction of the counters, claim races between neighbouring lanes."""
    keys = generic_keys(61, 65536)
    vals = values(np.random.default_rng(62), 65536)
    ends = []
    for dev in ("cpu", "cuda:0"):
        src = new_agent(pkg, dev, 18, True)
        src.import_rows(keys, vals)
        dst = new_agent(pkg, dev, 21, False)
        out = dst.unfold_from(src, mode="add", weight=0.25)
        sync(dev)
        k, q = dst.export_rows()
        order = np.argsort(k)
        ends.append((out, k[order], q[order].view(np.uint32)))
    assert ends[0][0] == ends[1][0] == {"read": 65536, "skipped": 0, "written": 524288, "created": 524288, "combined": 0,
                                        "dropped": 0}
    assert len(np.unique(ends[1][1])) == 524288
    assert np.array_equal(ends[0][1], ends[1][1]) and np.array_equal(ends[0][2], ends[1][2])
