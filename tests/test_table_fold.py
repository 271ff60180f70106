"""Folding a plain Q-table into a symmetry-folded one: q2048_table_fold, BatchedQLearningAgent.fold_from,
merge_tables.py --fold, train.py --resume PLAIN --symmetric --fold.

The checking model is independent numpy: a key is unpacked into a 4x4 array, its images are np.rot90 / np.fliplr as
include/q2048.h states them, the action permutation is the header's table copied by hand, and every float32 sum and
product is a numpy operation of its own.  It never calls q2048_canonicalize.  Rows are compared AS BIT PATTERNS, no
tolerance anywhere.  Every test runs on the CPU twin ("cpu") and on the GPU."""
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
FOLDS = ["mean", "mean_trained", "sum", "maxabs"]
MODES = [("add", 1.0), ("add", 0.25), ("blend", 0.3), ("maxabs", 1.0)]
MERGE_ID = {"add": 0, "blend": 1, "maxabs": 2}
FOLD_ID = {"mean": 0, "mean_trained": 1, "sum": 2, "maxabs": 3}
# pi_g(a), include/q2048.h (Q2048_FLAG_SYMMETRIC), row g, column a -- copied from the header's table
PI = [[0, 1, 2, 3], [3, 0, 1, 2], [2, 3, 0, 1], [1, 2, 3, 0], [2, 1, 0, 3], [1, 0, 3, 2], [0, 3, 2, 1], [3, 2, 1, 0]]
F32 = np.float32


def sync(dev):
    if dev != "cpu":
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


def to_canonical_frame(key, q):
    g = canon(key)[1]
    qc = np.zeros(4, F32)
    for a in range(4):
        qc[PI[g][a]] = q[a]
    return qc


def model_fold(src, fold):
    """src: {key: float32[4]} -> {canonical key: the orbit's row}; float32 operations one at a time."""
    out = {}
    for c in sorted({canon(k)[0] for k in src}):
        rows = [to_canonical_frame(m, src[m]) for m in members(c) if m in src]
        r = np.zeros(4, F32)
        for b in range(4):
            acc, n = F32(0.0), 0
            for row in rows:
                x = F32(row[b])
                if fold == "mean_trained" and x == 0:
                    continue
                if n == 0:
                    acc = x
                elif fold == "maxabs":
                    acc = x if np.abs(x) > np.abs(acc) else acc
                else:
                    acc = F32(acc + x)
                n += 1
            if fold in ("mean", "mean_trained"):
                acc = F32(acc * F32(1.0 / n)) if n else F32(0.0)
            r[b] = acc
        out[c] = r
    return out


def model_into(dst, folded, mode, w):
    """dst: {key: row} before; folded: model_fold's rows.  Returns (rows after, created, combined): the merge's
    formulas with the orbit's row as the source row, 1 - w computed once in float32."""
    w32 = F32(w)
    keep = F32(F32(1.0) - w32)
    out, created, combined = dict(dst), 0, 0
    with np.errstate(all="ignore"):
        for c, r in folded.items():
            if c not in dst:
                created += 1
                out[c] = (w32 * r).astype(F32) if mode == "add" else r.copy()
                continue
            combined += 1
            d = dst[c]
            if mode == "add":
                ws = (w32 * r).astype(F32)
                out[c] = (d + ws).astype(F32)
            elif mode == "blend":
                a, b = (keep * d).astype(F32), (w32 * r).astype(F32)
                out[c] = (a + b).astype(F32)
            else:
                out[c] = np.where(np.abs(r) > np.abs(d), r, d).astype(F32)
    return out, created, combined


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
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), \
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
MIRROR_BOTH = [[1, 2, 2, 1], [3, 4, 4, 3], [3, 4, 4, 3], [1, 2, 2, 1]]      # ... and to its np.flipud: 2 images
DIAGONALS = [[1, 2, 3, 4], [2, 5, 6, 3], [3, 6, 5, 2], [4, 3, 2, 1]]        # equal to its transpose and anti-transpose: 2
ALL_EQUAL = [[3] * 4] * 4                                                   # 1 image
ALL_SYMMETRIC = [[1, 2, 2, 1], [2, 3, 3, 2], [2, 3, 3, 2], [1, 2, 2, 1]]    # equal to transpose and mirror: 1 image
# which members (indices into members(c)) have a row: all 8; k = 1, 2, 3, 5, 7 with the canonical member (index 0)
# absent in several, and lone members whose own g is >= 4 (a mirror image is its own inverse)
SHAPES8 = [tuple(range(8)), (0,), (2,), (5,), (7,), (1, 6), (0, 4), (0, 3, 4), (2, 5, 6), (1, 2, 4, 5, 7),
           (0, 1, 3, 5, 6), tuple(range(1, 8)), (0, 1, 2, 3, 4, 5, 6)]


def orbit_values(rng, k):
    """k rows in the CANONICAL frame: random float32 of both signs, exact +0.0 and -0.0 entries, now and then a
    column that is zero in every member, and columns of equal magnitude with mixed signs (the MAXABS tie)."""
    v = (rng.standard_normal((k, 4)) * 10.0).astype(F32)
    zero = rng.random((k, 4))
    v[zero < 0.25] = F32(0.0)
    v[(zero >= 0.25) & (zero < 0.35)] = F32(-0.0)
    if rng.random() < 0.4:
        v[:, rng.integers(4)] = np.where(rng.random(k) < 0.5, F32(0.0), F32(-0.0))
    if rng.random() < 0.5:
        v[:, rng.integers(4)] = F32(rng.standard_normal() * 5.0) * np.where(rng.random(k) < 0.5, F32(1.0), F32(-1.0))
    return v


def source_of(rng, orbits):
    """orbits: [(canonical key, member indices)] -> {key: row in the member's OWN frame}."""
    src = {}
    for c, shape in orbits:
        ms = members(c)
        vals = orbit_values(rng, len(shape))
        for j, h in enumerate(shape):
            g = canon(ms[h])[1]
            src[ms[h]] = np.array([vals[j][PI[g][a]] for a in range(4)], F32)
    return src


_HAND = {}


def hand_built(seed=7, per_shape=4):
    """The hand-built source of tests 2, 4 and 5 (built once): generic orbits in every SHAPES8 shape, and the
    stabiliser boards with all and with some of their members present."""
    if (seed, per_shape) not in _HAND:
        rng = np.random.default_rng(seed)
        orbits = [(generic_board(rng), shape) for shape in SHAPES8 for _ in range(per_shape)]
        for board, count in ((MIRROR, 4), (MIRROR_BOTH, 2), (DIAGONALS, 2), (ALL_EQUAL, 1), (ALL_SYMMETRIC, 1)):
            for shift in range(3):                                   # three orbits of the same symmetry
                c = canon(pack((np.array(board) + shift) % 16))[0]
                assert len(members(c)) == count
                shape = tuple(range(count)) if shift == 0 else tuple(range(count))[(shift % count):][:max(1, count - 1)]
                orbits.append((c, shape))
        assert len({c for c, _ in orbits}) == len(orbits)
        lone = [canon(members(c)[s[0]])[1] for c, s in orbits if len(s) == 1 and len(members(c)) == 8]
        assert max(lone) >= 4 and any(0 not in s for _, s in orbits)
        _HAND[(seed, per_shape)] = (orbits, source_of(rng, orbits))
    return _HAND[(seed, per_shape)]


def check_fold(pkg, dst, src, fold, mode, w, what=""):
    """fold_from against the model, with the identities the counters and the bookkeeping owe."""
    before, other = as_dict(dst.export_rows()), as_dict(src.export_rows())
    size_before = dst.table_size()
    src_table = src.table.clone()
    out = dst.fold_from(src, fold=fold, mode=mode, weight=w)
    sync(dst.device.type)
    folded = model_fold(other, fold)
    want, created, combined = model_into(before, folded, mode, w)
    assert out["read"] == len(other) and out["orbits"] == len(folded), (what, out)
    assert out["dropped"] == 0 and out["created"] == created and out["combined"] == combined, (what, out, created, combined)
    assert out["orbits"] == out["created"] + out["combined"] + out["dropped"]
    assert dst.table_size() == size_before + created
    dst.verify_table()
    assert torch.equal(src.table, src_table), "the source was written"
    assert_same(as_dict(dst.export_rows()), want, what)
    return out, want


# ---------------------------------------------------------------------------------------------
# 1. symbol and signature
# ---------------------------------------------------------------------------------------------
def test_both_libraries_export_the_fold(pkg):
    N = pkg._native
    assert "q2048_table_fold" in N._SIGNATURES
    assert (N.FOLD_MEAN, N.FOLD_MEAN_TRAINED, N.FOLD_SUM, N.FOLD_MAXABS) == (0, 1, 2, 3)
    assert hasattr(C.CDLL(N.HOST_LIB_PATH), "q2048_table_fold")
    assert hasattr(C.CDLL(N.LIB_PATH), "q2048_table_fold")           # loads without a GPU: no compute call here
    assert N.host_lib().q2048_abi_version() == N.lib().q2048_abi_version() == 7   # additive: detected by its symbol
    with open(os.path.join(REPO, "include", "q2048.h")) as fh:
        hdr = fh.read()
    for name, value in (("Q2048_FOLD_MEAN", 0), ("Q2048_FOLD_MEAN_TRAINED", 1), ("Q2048_FOLD_SUM", 2), ("Q2048_FOLD_MAXABS", 3)):
        assert f"#define {name} {value}\n" in hdr
    # the model's permutation table is the header's formula
    for g in range(8):
        for a in range(4):
            assert PI[g][a] == ((a - g) & 3 if g < 4 else (2 - a - (g - 4)) & 3)


# ---------------------------------------------------------------------------------------------
# 2. hand-built orbits, every fold and mode
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("fold", FOLDS)
@pytest.mark.parametrize("mode,w", MODES)
def test_hand_built_orbits_equal_the_model(pkg, dev, fold, mode, w):
    orbits, rows = hand_built()
    src = agent_with(pkg, dev, 10, False, rows)
    dst = new_agent(pkg, dev, 10, True)
    out, want = check_fold(pkg, dst, src, fold, mode, w, f"{fold} {mode} w={w}")
    assert out["orbits"] == out["created"] == len(orbits) and out["read"] == len(rows) and out["combined"] == 0
    if fold == "mean_trained":                       # the source exercises the rule: an all-untrained column reads +0
        assert any((r.view(np.uint32) == 0).any() for r in want.values())


# ---------------------------------------------------------------------------------------------
# 3. the frame's direction, without the model
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("g", [1, 5])
def test_frame_direction(pkg, dev, g):
    """One row m -> [1, 2, 3, 4] with m a non-canonical board whose canonical image is image_g(m).  The folded agent
    answers in the env's frame: board m reads [1, 2, 3, 4] again, the canonical board reads the row as it is stored."""
    c = generic_board(np.random.default_rng(3))
    m = next(k for k in members(c) if canon(k)[1] == g)
    assert m != c and pack(images(unpack(m))[g]) == c
    row = np.array([1.0, 2.0, 3.0, 4.0], F32)
    src = agent_with(pkg, dev, 8, False, {m: row})
    dst = new_agent(pkg, dev, 8, True)
    out = dst.fold_from(src, fold="mean")
    assert out == {"read": 1, "orbits": 1, "created": 1, "combined": 0, "dropped": 0}
    boards = torch.from_numpy(np.stack([unpack(m).reshape(16), unpack(c).reshape(16)])).to(dev)
    got = dst.q_values(boards).cpu().numpy()
    stored = np.zeros(4, F32)
    for a in range(4):
        stored[PI[g][a]] = row[a]                    # Q_canon[pi_g(a)] = Q_m[a]
    assert np.array_equal(got[0], row), got
    assert np.array_equal(got[1], stored), got       # (the canonical board's own g is 0: env frame = canonical frame)
    assert as_dict(dst.export_rows()).keys() == {c}


# ---------------------------------------------------------------------------------------------
# 4. a destination that already holds rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("fold,mode,w", [("mean", "add", 1.0), ("mean_trained", "add", 0.25), ("sum", "blend", 0.3),
                                         ("maxabs", "maxabs", 1.0), ("maxabs", "blend", 1.0)])
def test_prefilled_destination(pkg, dev, fold, mode, w):
    orbits, rows = hand_built()
    rng = np.random.default_rng(11)
    held = {c: orbit_values(rng, 1)[0] for c, _ in orbits[::2]}                     # half of the orbits have a row
    others = {}
    while len(others) < 40:                                                         # orbits the source never touches
        c = generic_board(rng)
        if c not in {o for o, _ in orbits}:
            others[c] = orbit_values(rng, 1)[0]
    src = agent_with(pkg, dev, 10, False, rows)
    dst = agent_with(pkg, dev, 10, True, {**held, **others})
    out, _ = check_fold(pkg, dst, src, fold, mode, w, f"{fold} {mode} w={w}")
    assert out["combined"] == len(held) and out["created"] == len(orbits) - len(held)
    after = as_dict(dst.export_rows())
    for c, r in others.items():
        assert np.array_equal(after[c].view(np.uint32), r.view(np.uint32))


# ---------------------------------------------------------------------------------------------
# 5. probe and stride edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_small_source_at_load_080(pkg, dev):
    """2^8 slots, 205 rows: the member lookups wrap around the table's end and walk chains."""
    rng = np.random.default_rng(21)
    shapes = [SHAPES8[i % len(SHAPES8)] for i in range(200)]
    orbits, total = [], 0
    for shape in shapes:
        if total + len(shape) > 205:
            shape = (int(rng.integers(8)),)
        if total + len(shape) > 205:
            break
        orbits.append((generic_board(rng), shape))
        total += len(shape)
    rows = source_of(rng, orbits)
    assert len(rows) == 205
    src = agent_with(pkg, dev, 8, False, rows)
    assert src.capacity_log2 == 8 and src.table_size() == 205
    for fold in ("mean", "maxabs"):
        check_fold(pkg, new_agent(pkg, dev, 10, True), src, fold, "add", 1.0, f"load 0.8, {fold}")


@pytest.mark.parametrize("dev", DEVICES)
def test_source_larger_than_one_grid_pass(pkg, dev):
    """The launch caps its grid at 2048 blocks of 256 lanes: a 2^20-slot source takes two passes of the grid-stride
    loop, and an orbit's members lie in different passes and blocks."""
    orbits, rows = hand_built()
    src = agent_with(pkg, dev, 20, False, rows)
    slots = torch.nonzero(src.table.view(torch.int64).reshape(-1, 4)[:, 0] != 0).reshape(-1)
    assert int((slots >= (1 << 19)).sum()) > 20 and int((slots < (1 << 19)).sum()) > 20
    check_fold(pkg, new_agent(pkg, dev, 10, True), src, "mean_trained", "add", 1.0, "2^20-slot source")


@pytest.mark.parametrize("dev", DEVICES)
def test_destination_at_load_085_equals_a_roomy_one(pkg, dev):
    rng = np.random.default_rng(31)
    orbits = [(generic_board(rng), (int(rng.integers(8)),)) for _ in range(206)]
    orbits += [(generic_board(rng), (int(rng.integers(4)), int(rng.integers(4, 8)))) for _ in range(12)]
    rows = source_of(rng, orbits)
    assert len(orbits) == 218 and len(rows) == 230
    src = agent_with(pkg, dev, 10, False, rows)
    tight, roomy = new_agent(pkg, dev, 8, True), new_agent(pkg, dev, 12, True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                # (no deep row: the probe limit is the table)
        _, want = check_fold(pkg, tight, src, "mean", "add", 0.25, "load 0.85")
        check_fold(pkg, roomy, src, "mean", "add", 0.25, "roomy")
    assert tight.table_size() == 218 and tight.capacity_log2 == 8    # 218 / 256 = 0.85
    assert_same(as_dict(tight.export_rows()), as_dict(roomy.export_rows()), "tight against roomy")


# ---------------------------------------------------------------------------------------------
# 6. a trained table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_trained_table(pkg, dev):
    env = pkg.BatchedGame2048Env(256, board_size=4, seed=1, env_id0=0, device=dev)
    plain = new_agent(pkg, dev, 16, False)
    for _ in range(3):
        plain.fused_rollout(env, 10)
    sync(dev)
    assert plain.check_status() == 0
    folded = new_agent(pkg, dev, 16, True)
    out, want = check_fold(pkg, folded, plain, "maxabs", "add", 1.0, "trained table")
    assert 0 < out["created"] < out["read"]                          # mirror images were met: the table shrank
    assert all(canon(k)[0] == k for k in want)
    env2 = pkg.BatchedGame2048Env(256, board_size=4, seed=1, env_id0=0, device=dev)
    folded.epsilon = 0.0
    folded.fused_rollout(env2, 10)
    sync(dev)
    assert folded.check_status() == 0
    s = folded.stats(verify=True)
    assert s["steps"] == 256 * 10 and s["drops"] == 0


# ---------------------------------------------------------------------------------------------
# 7. argument errors; the agent's refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["hip", "host"])
def test_abi_argument_errors(pkg, which):
    """One call per error, fake aligned addresses otherwise: validation runs on the host before anything is launched
    (or, on the CPU twin, touched)."""
    N = pkg._native
    L = N.lib() if which == "hip" else N.host_lib()
    f = L.q2048_table_fold
    d, s, c, st = 1 << 30, 1 << 40, 1 << 20, 1 << 21
    NULL, SIZE, ALIGN, UNSUPPORTED, RANGE, FLAGS = -1, -2, -3, -4, -6, -7
    assert f(None, 20, s, 20, 1, 0, 0, 1.0, c, st, None) == NULL
    assert f(d, 20, None, 20, 1, 0, 0, 1.0, c, st, None) == NULL
    assert f(d, 20, s, 20, 1, 0, 0, 1.0, None, st, None) == NULL
    assert f(d, 20, s, 20, 2, 0, 0, 1.0, c, st, None) == UNSUPPORTED          # 5x5
    assert f(d, 20, s, 20, 0, 0, 0, 1.0, c, st, None) == SIZE
    assert f(d, 20, s, 20, 3, 0, 0, 1.0, c, st, None) == SIZE
    assert f(d, 3, s, 20, 1, 0, 0, 1.0, c, st, None) == SIZE
    assert f(d, 41, s, 20, 1, 0, 0, 1.0, c, st, None) == SIZE
    assert f(d, 20, s, 3, 1, 0, 0, 1.0, c, st, None) == SIZE
    assert f(d, 20, s, 41, 1, 0, 0, 1.0, c, st, None) == SIZE
    assert f(d + 8, 20, s, 20, 1, 0, 0, 1.0, c, st, None) == ALIGN
    assert f(d, 20, s + 8, 20, 1, 0, 0, 1.0, c, st, None) == ALIGN
    assert f(d, 20, s, 20, 1, 4, 0, 1.0, c, st, None) == FLAGS
    assert f(d, 20, s, 20, 1, -1, 0, 1.0, c, st, None) == FLAGS
    assert f(d, 20, s, 20, 1, 0, 3, 1.0, c, st, None) == FLAGS
    assert f(d, 20, s, 20, 1, 0, -1, 1.0, c, st, None) == FLAGS
    assert f(d, 20, s, 20, 1, 0, 0, float("nan"), c, st, None) == RANGE
    assert f(d, 20, s, 20, 1, 3, 2, float("inf"), c, st, None) == RANGE
    assert f(d, 20, s, 20, 1, 0, 1, 1.5, c, st, None) == RANGE
    assert f(d, 20, s, 20, 1, 0, 1, -0.25, c, st, None) == RANGE
    assert f(d, 20, d, 20, 1, 0, 0, 1.0, c, st, None) == RANGE                       # src == dst
    assert f(d, 20, d + (32 << 20) - 32, 20, 1, 0, 0, 1.0, c, st, None) == RANGE     # the last slot of dst is src's first
    assert f(d + (32 << 16) - 32, 20, d, 16, 1, 0, 0, 1.0, c, st, None) == RANGE     # ... and the other way round
    # the order: NULL, UNSUPPORTED, SIZE, ALIGN, FLAGS, RANGE (w), RANGE (overlap)
    assert f(None, 99, s + 8, 20, 2, 9, 9, float("nan"), c, st, None) == NULL
    assert f(d + 8, 99, s, 20, 2, 9, 9, float("nan"), c, st, None) == UNSUPPORTED
    assert f(d + 8, 99, s, 20, 1, 9, 9, float("nan"), c, st, None) == SIZE
    assert f(d + 8, 20, s, 20, 1, 9, 9, float("nan"), c, st, None) == ALIGN
    assert f(d, 20, s, 20, 1, 9, 0, float("nan"), c, st, None) == FLAGS
    assert f(d, 20, s, 20, 1, 0, 9, float("nan"), c, st, None) == FLAGS
    assert f(d, 20, d, 20, 1, 0, 0, float("nan"), c, st, None) == RANGE


@pytest.mark.parametrize("dev", DEVICES)
def test_through_ctypes_the_source_is_only_read(pkg, dev):
    """The raw call: counters are added to, `src` keeps every byte -- line summaries in its spare words included --
    and the `reserved` words of `dst` stay what they were."""
    N = pkg._native
    orbits, rows = hand_built()
    src = agent_with(pkg, dev, 10, False, rows)
    N.check(src._L.q2048_table_summarise(src.table.data_ptr(), 10, None), "table_summarise")
    dst = new_agent(pkg, dev, 10, True)
    sync(dev)
    before = src.table.clone()
    assert bool((before.view(torch.int64).reshape(-1, 4)[:, 3] != 0).any())          # the summaries are there
    counters = torch.tensor([5, 4, 3, 2, 1], dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    N.check(dst._L.q2048_table_fold(dst.table.data_ptr(), 10, src.table.data_ptr(), 10, 1, FOLD_ID["sum"], MERGE_ID["blend"],
                                    0.3, counters.data_ptr(), status.data_ptr(), None), "table_fold")
    sync(dev)
    assert torch.equal(src.table, before)
    assert counters.tolist() == [5 + len(rows), 4 + len(orbits), 3 + len(orbits), 2, 1] and int(status.item()) == 0
    assert not bool((dst.table.view(torch.int64).reshape(-1, 4)[:, 3] != 0).any())
    dst.recount_rows()
    want, _, _ = model_into({}, model_fold(rows, "sum"), "blend", 0.3)
    assert_same(as_dict(dst.export_rows()), want, "raw call")
    # 5x5 tables are refused before anything is touched
    code = dst._L.q2048_table_fold(dst.table.data_ptr(), 10, src.table.data_ptr(), 10, 2, 0, 0, 1.0, counters.data_ptr(),
                                   status.data_ptr(), None)
    assert code == -4                                                                # Q2048_ERR_UNSUPPORTED


@pytest.mark.parametrize("dev", DEVICES)
def test_agent_refusals(pkg, dev):
    plain, other_plain = new_agent(pkg, dev, 8, False), new_agent(pkg, dev, 8, False)
    folded, other_folded = new_agent(pkg, dev, 8, True), new_agent(pkg, dev, 8, True)
    with pytest.raises(ValueError, match="already symmetry-folded"):
        folded.fold_from(other_folded)
    with pytest.raises(ValueError, match="symmetry-folded destination"):
        plain.fold_from(other_plain)
    with pytest.raises(ValueError):
        folded.fold_from(folded)
    five = pkg.BatchedQLearningAgent(10, capacity_log2=8, device=dev, board_size=5, placement="plain", freeze_load=None)
    with pytest.raises(ValueError, match="board size 4"):
        folded.fold_from(five)
    salted = new_agent(pkg, dev, 8, False, independent=True)
    with pytest.raises(ValueError, match="independent"):
        folded.fold_from(salted)
    with pytest.raises(ValueError, match="independent"):
        new_agent(pkg, dev, 8, True, independent=True).fold_from(plain)
    with pytest.raises(ValueError, match="fold must be"):
        folded.fold_from(plain, fold="median")
    with pytest.raises(ValueError, match="mode"):
        folded.fold_from(plain, mode="mean")
    with pytest.raises(ValueError, match="weight"):
        folded.fold_from(plain, mode="blend", weight=1.5)
    if dev != "cpu":
        with pytest.raises(ValueError, match="different devices"):
            folded.fold_from(new_agent(pkg, "cpu", 8, False))
    # the mix stays refused where no fold was asked for
    with pytest.raises(ValueError, match="folded"):
        folded.merge_from(plain)
    with pytest.raises(ValueError, match="folded"):
        folded.load_state_dict(plain.state_dict())
    # a destination whose key set is closed refuses
    env = pkg.BatchedGame2048Env(512, board_size=4, seed=1, env_id0=0, device=dev)
    frozen = new_agent(pkg, dev, 10, True, freeze_load=0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(6):
            frozen.fused_rollout(env, 20)
    sync(dev)
    assert frozen.frozen
    with pytest.raises(ValueError, match="closed"):
        frozen.fold_from(plain)
    # too small: refused before anything is launched
    _, rows = hand_built()
    tiny = new_agent(pkg, dev, 6, True)
    with pytest.raises(ValueError, match="too small"):
        tiny.fold_from(agent_with(pkg, dev, 10, False, rows))
    assert tiny.table_size() == 0


# ---------------------------------------------------------------------------------------------
# 8. the scripts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_scripts_fold(pkg, dev, tmp_path):
    device = "cpu" if dev == "cpu" else "cuda"
    py = lambda script, *a: subprocess.run([sys.executable, os.path.join(REPO, script), "--device", device, *a],   # noqa: E731
                                           capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    small = ("--num-envs", "64", "--steps-per-launch", "16", "--max-steps", "32", "--capacity-log2", "16")
    for seed in (1, 2):
        p = py("train.py", *small, "--episodes", "2", "--seed", str(seed), "--save", f"q{seed}.pt", "--log", f"log{seed}.csv")
        assert p.returncode == 0, p.stderr[-2000:]
    p = py("train.py", *small, "--episodes", "2", "--seed", "3", "--symmetric", "--save", "f3.pt", "--log", "log3.csv")
    assert p.returncode == 0, p.stderr[-2000:]
    a, b, f3 = (torch.load(tmp_path / f, map_location="cpu", weights_only=False) for f in ("q1.pt", "q2.pt", "f3.pt"))
    assert "symmetric" not in a and f3["symmetric"] is True

    # two plain files -> one folded file: the mean over the inputs of each input's maxabs fold
    p = py("merge_tables.py", "--fold", "maxabs", "--mode", "mean", "--out", "folded.pt", "q1.pt", "q2.pt")
    assert p.returncode == 0, p.stderr[-2000:]
    report = json.loads(p.stdout.strip().splitlines()[-1])
    m = torch.load(tmp_path / "folded.pt", map_location="cpu", weights_only=False)
    assert m["symmetric"] is True and m["merged"]["fold"] == "maxabs" and m["merged"]["mode"] == "mean"
    want, c1, _ = model_into({}, model_fold(as_dict((a["keys"], a["q"])), "maxabs"), "add", 0.5)
    want, c2, s2 = model_into(want, model_fold(as_dict((b["keys"], b["q"])), "maxabs"), "add", 0.5)
    assert_same(as_dict((m["keys"], m["q"])), want, "merge_tables.py --fold maxabs")
    assert report["fold"] == "maxabs" and report["rows_out"] == len(want)
    assert [(r["read"], r["created"], r["combined"]) for r in report["merges"]] == [(len(a["q"]), c1, 0), (len(b["q"]), c2, s2)]
    p = py("evaluate.py", "--model", "folded.pt", "--num-envs", "64", "--episodes", "1", "--max-steps", "32")
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["rows"] == len(want) and res["symmetric"] is True

    # one plain input: the converter
    p = py("merge_tables.py", "--fold", "mean_trained", "--mode", "sum", "--out", "one.pt", "q1.pt")
    assert p.returncode == 0, p.stderr[-2000:]
    one = torch.load(tmp_path / "one.pt", map_location="cpu", weights_only=False)
    want1, _, _ = model_into({}, model_fold(as_dict((a["keys"], a["q"])), "mean_trained"), "add", 1.0)
    assert one["symmetric"] is True
    assert_same(as_dict((one["keys"], one["q"])), want1, "the converter")

    # a mixed pair: accepted with --fold (the folded input merges as it is), refused without
    p = py("merge_tables.py", "--fold", "mean", "--mode", "sum", "--out", "mixed.pt", "f3.pt", "q1.pt")
    assert p.returncode == 0, p.stderr[-2000:]
    mixed = torch.load(tmp_path / "mixed.pt", map_location="cpu", weights_only=False)
    wantm, _, _ = model_into({}, as_dict((f3["keys"], f3["q"])), "add", 1.0)
    wantm, _, _ = model_into(wantm, model_fold(as_dict((a["keys"], a["q"])), "mean"), "add", 1.0)
    assert mixed["symmetric"] is True and mixed["merged"]["folded_inputs"] == ["q1.pt"]
    assert_same(as_dict((mixed["keys"], mixed["q"])), wantm, "a mixed pair")
    p = py("merge_tables.py", "--mode", "sum", "--out", "bad.pt", "f3.pt", "q1.pt")
    assert p.returncode != 0 and "cannot be merged" in p.stderr and not (tmp_path / "bad.pt").exists()

    # train.py --resume PLAIN --symmetric --fold: one more epoch on the folded table
    resume = ("train.py", *small, "--episodes", "3", "--seed", "1", "--resume", "q1.pt", "--symmetric", "--log", "log4.csv")
    p = py(*resume, "--fold", "maxabs", "--save", "r.pt")
    assert p.returncode == 0, p.stderr[-2000:]
    r = torch.load(tmp_path / "r.pt", map_location="cpu", weights_only=False)
    assert r["symmetric"] is True and r["train"]["epoch"] >= a["train"]["epoch"] and "visit_rows" not in r
    assert all(canon(k)[0] == k for k in r["keys"].tolist())
    assert int(r["stats_i"][0]) > int(a["stats_i"][0])                               # the statistics went on
    p = py(*resume)
    assert p.returncode != 0 and "do not load into each other" in p.stderr           # the refusal of today
    p = py(*resume[:-3], "--log", "log5.csv", "--fold", "maxabs")                    # (no --symmetric)
    assert p.returncode != 0 and "--symmetric" in p.stderr
    p = py("train.py", *small, "--episodes", "3", "--seed", "3", "--resume", "f3.pt", "--symmetric", "--fold", "maxabs",
           "--log", "log6.csv")
    assert p.returncode != 0 and "already" in p.stderr
