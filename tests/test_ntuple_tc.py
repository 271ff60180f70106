"""Temporal-coherence step sizes for the 6-tuple afterstate network (q2048_nt_tc_update, q2048_nt_tc_fused_rollout):
V = float32 [4, 2^24] beside acc = float32 [4, 2^24, 2] of pairs {E, A}, against a numpy model that extends
test_ntuple's `model_update` with the rule of include/q2048.h, and BatchedNTupleAgent(coherence=True) with its
checkpoint.  (The scripts: test_ntuple_tc_scripts.py.)

Which test executes which kernel (device) / function (CPU twin):
  k_nt_tc_update         test_update_where_lanes_cannot_race, test_zero_history_is_the_plain_step, test_symmetric_boards,
                         the loop of test_fused_one_lane_many_steps
  k_nt_tc_fused_rollout  test_fused_one_lane_many_steps, test_fused_one_learning_step, test_lr_zero_accumulates_only,
                         test_racing_at_65536_boards_properties, the checkpoint tests
  the argument checks    test_abi, test_argument_errors_need_no_device, test_refused_calls_write_nothing

Every comparison is exact and over ALL of V (256 MiB) and ALL of acc (512 MiB), as float32 bit patterns.  There is no
tolerance: the rate is one float32 division and a float32 minimum, d_i one float64 expression rounded once
(lr * 0.03125 is exact), and the two sums of a pair one float32 addition each.  The base accumulators carry a history
on every entry: a quarter each of A = 0, |E| = A (rate 1), 0 < |E| < A and E = 0 < A (rate 0); the tests assert that the
entries they visit hold all four."""
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
base_values, base_on = NT.base_values, NT.base_on
NAMES = ("q2048_nt_tc_update", "q2048_nt_tc_fused_rollout")
V_BYTES, ACC_BYTES = 1 << 28, 1 << 29
_SHARED = {}


# ---------------------------------------------------------------------------------------------------------------
# the base accumulators and the model
# ---------------------------------------------------------------------------------------------------------------
def base_acc():
    """float32 [4, 2^24, 2], a function of the bits of `base_values()`, built once per module; nobody writes it.  By two
    bits of the value: A = 0 (no history); |E| = A; 0 < |E| < A (E = +-A * u, u in [0.05, 0.95]: the float32 product stays
    below A); E = 0 < A.  A = |value| + 0.5, the sign of E is another bit."""
    if "acc" not in _SHARED:
        v = base_values()
        vb = bits(v)
        cat = (vb >> 5) & 3
        A = np.abs(v) + F32(0.5)
        u = ((vb >> 7) & 0xff).astype(F32) * F32(0.9 / 256) + F32(0.05)
        E = np.where(cat == 1, A, np.where(cat == 2, A * u, F32(0.0))).astype(F32)
        E = np.where((vb >> 4) & 1, -E, E)
        acc = np.stack([E, np.where(cat == 0, F32(0.0), A)], axis=-1).astype(F32)
        assert acc.shape == (4, NIDX, 2) and (np.abs(acc[..., 0]) <= acc[..., 1]).all()
        acc.setflags(write=False)
        _SHARED["acc"] = acc
    return _SHARED["acc"]


def acc_on(dev):
    """The base accumulators on `dev`, uploaded once per device for the tests that must NOT write them."""
    key = ("t", str(dev))
    if key not in _SHARED:
        _SHARED[key] = t32(dev, base_acc())
    return _SHARED[key]


def categories(acc, ids):
    """How many of the entries `ids` (p * 2^24 + idx) hold A = 0, |E| = A > 0, 0 < |E| < A, E = 0 < A."""
    h = acc.reshape(-1, 2)[np.unique(ids)]
    E, A = np.abs(h[:, 0]), h[:, 1]
    return [int((A == 0).sum()), int(((A > 0) & (E == A)).sum()), int(((E > 0) & (E < A)).sum()), int(((A > 0) & (E == 0)).sum())]


def model_rate(E, A):
    """r = (A > 0) ? fminf(fabsf(E) / A, 1) : 1 -- float32; fmin returns the other operand for a NaN"""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(A > 0, np.fmin(np.abs(E) / A, F32(1.0)), F32(1.0))
    assert r.dtype == F32
    return r


def model_tc_update(O, V, acc, s, actions, s2, done, lr, gamma, inplace=False):
    """test_ntuple.model_update with the rule: lane after lane on one pair of arrays, the 32 entries and the 32 pairs
    gathered, then each entry written as gathered + d_i and each pair as gathered + {e, |e|}.
    -> (values, accumulators, status word, int [B, 4, 8] written indices or -1, float32 [B] e)"""
    V, acc, status = (V if inplace else V.copy()), (acc if inplace else acc.copy()), 0
    written = np.full((len(s), 4, 8), -1, np.int64)
    es = np.zeros(len(s), F32)
    pp = np.arange(4)[:, None]
    for i in range(len(s)):
        a = int(actions[i])
        if a > 3:
            status |= BAD_ACTION
            continue
        x, _, legal = O.move(s[i], a)
        if not legal:
            continue
        q2, legal2, _ = NT.model_eval(O, V, s2[i:i + 1])
        live = 1.0 if (not done[i]) and legal2.any() else 0.0
        target = (gamma * float(NT.model_best(q2, legal2)[0])) * live                # float64
        err = target - float(NT.model_v(V, x[None])[0])                              # float64
        e = F32(err)                                                                  # rounded once
        idx = NT.model_idx(x[None])[0]
        gathered, h = V[pp, idx], acc[pp, idx]                                        # [4, 8], [4, 8, 2]
        E, A = h[..., 0], h[..., 1]
        d = (((lr * 0.03125) * err) * model_rate(E, A).astype(np.float64)).astype(F32)
        V[pp, idx] = gathered + d
        acc[pp, idx, 0] = E + e
        acc[pp, idx, 1] = A + np.abs(e)
        written[i], es[i] = idx, e
    return V, acc, status, written, es


def ids_of(written):
    """entry ids p * 2^24 + idx of the lanes that wrote -> 1-D int64 with repeats"""
    w = written[written[:, 0, 0] >= 0]
    return (w + (np.arange(4) * NIDX)[None, :, None]).ravel()


def changed_pairs(acc, base):
    return int(np.count_nonzero((bits(acc) != bits(base)).any(axis=-1)))


def assert_coherent(acc, what):
    """finite, A >= 0 and |E| <= A exactly, over all 2^26 pairs"""
    acc = acc.cpu().numpy() if isinstance(acc, torch.Tensor) else acc
    E, A = acc[..., 0], acc[..., 1]
    assert np.isfinite(acc).all(), f"{what}: a pair is not finite"
    assert (A >= 0).all() and (np.abs(E) <= A).all(), f"{what}: {int((np.abs(E) > A).sum())} pairs with |E| > A"


def tc_update(L, dev, weights, acc, s, actions, s2, done, lr, gamma):
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ts, ts2, ta, td = t8(dev, s), t8(dev, s2), t8(dev, actions), t8(dev, done)
    assert L.q2048_nt_tc_update(weights.data_ptr(), acc.data_ptr(), ts.data_ptr(), ta.data_ptr(), ts2.data_ptr(),
                                td.data_ptr(), len(s), lr, gamma, status.data_ptr(), None) == 0
    for t, a in ((ts, s), (ts2, s2), (ta, actions), (td, done)):
        assert np.array_equal(t.cpu().numpy(), a), "an input was written"
    return int(status.item())


def make_agent(pkg, dev, eps=0.3, lr=0.1, gamma=0.95, seed=P.SEED, id0=P.ID0, epochs=100, coherence=True):
    return pkg.BatchedNTupleAgent(epochs, learning_rate=lr, discount_factor=gamma, exploration_rate=eps, seed=seed,
                                  env_id0=id0, device=dev, coherence=coherence)


# ---------------------------------------------------------------------------------------------------------------
# 1. ABI and argument errors
# ---------------------------------------------------------------------------------------------------------------
def test_abi(pkg):
    N = pkg._native
    with open(os.path.join(REPO, "include", "q2048.h")) as fh:
        header = fh.read()
    for name, at in zip(NAMES, (1, 3)):                    # the counterpart's list with `acc` directly after `weights`
        assert name in N._SIGNATURES, name
        assert hasattr(N.host_lib(), name) and hasattr(N.lib(), name), name
        assert f"int {name}(" in header, name
        res, args = N._SIGNATURES[name.replace("_tc_", "_")]
        assert N._SIGNATURES[name] == (res, args[:at] + [args[at - 1]] + args[at:]), name
    assert N.host_lib().q2048_abi_version() == N.lib().q2048_abi_version() == N.ABI_VERSION
    assert issubclass(pkg.BatchedNTupleAgent, pkg.BatchedAfterstateAgent)


def entry_points(L):
    a = [(k + 1) << 32 for k in range(8)]                  # made-up addresses 4 GiB apart: V and acc do not overlap
    nan = float("nan")
    # name: (function, good arguments, required pointers, 16-byte aligned pointers, position of B, {scalar position: refused},
    #        positions of weights and acc)
    return {
        "nt_tc_update": (L.q2048_nt_tc_update, [a[0], a[6], a[1], a[2], a[3], a[4], 64, 0.1, 0.97, a[5], None],
                         (0, 1, 2, 3, 4, 5, 9), (0, 1, 2, 4), 6, {7: (nan,), 8: (nan,)}, (0, 1)),
        "nt_tc_fused_rollout": (L.q2048_nt_tc_fused_rollout, [a[0], a[1], a[2], a[6], 64, 2, 0.3, 0.1, 0.97, 3, 50, 0, None,
                                                              None, a[3], None],
                                (0, 1, 2, 3, 14), (0, 1, 2, 3), 4, {6: (-0.1, 1.5, nan), 7: (nan,), 8: (nan,)}, (2, 3)),
    }


@pytest.mark.parametrize("which", ["hip", "host"])
def test_argument_errors_need_no_device(pkg, which):
    """The order of the q2048_nt_* counterparts -- B, NULL, alignment, (steps,) the scalars -- with acc in the NULL and
    in the alignment list, and the overlap of V and acc refused with Q2048_ERR_RANGE after the alignment: on both
    libraries, with made-up addresses, so nothing behind them may be touched (B == 0 and steps == 0 are no-ops)."""
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
            kw = {**bad_align, **bad_scalar, f"p{pos}": None}
            assert call(**kw) == ERR_NULL, f"{name}: NULL in position {pos}"
        for pos in aligned:                                             # the alignment before the overlap and the scalars
            assert call(**{f"p{pos}": good[pos] + 8}, **bad_scalar) == ERR_ALIGN, f"{name}: position {pos} off by 8 bytes"
        for pos, values in scalars.items():
            for value in values:
                assert call(**{f"p{pos}": value}) == ERR_RANGE, f"{name}: {value} in position {pos}"
        assert call(**{f"p{b_pos}": 0}) == 0, f"{name}: B = 0"
        assert call(**{f"p{b_pos}": 0, f"p{pointers[0]}": None}) == ERR_NULL, f"{name}: B = 0 is checked first"
        # the overlap of [weights, weights + 256 MiB) and [acc, acc + 512 MiB): refused, B = 0 included; touching is fine
        w = good[w_pos]
        for acc, code in ((w, ERR_RANGE), (w + 16, ERR_RANGE), (w + V_BYTES - 16, ERR_RANGE), (w + V_BYTES, 0),
                          (w - 16, ERR_RANGE), (w - ACC_BYTES + 16, ERR_RANGE), (w - ACC_BYTES, 0)):
            assert call(**{f"p{acc_pos}": acc, f"p{b_pos}": 0}) == code, f"{name}: acc = weights {acc - w:+d}"
        assert call(**{f"p{acc_pos}": w}) == ERR_RANGE, f"{name}: acc == weights"
        assert call(**{f"p{acc_pos}": w + 8}) == ERR_ALIGN, f"{name}: the alignment before the overlap"
        assert call(**{f"p{acc_pos}": w, f"p{pointers[-1]}": None}) == ERR_NULL, f"{name}: NULL before the overlap"
    fn, good = table["nt_tc_fused_rollout"][:2]
    for steps, eps, code in ((-1, nan, ERR_SIZE), ((1 << 30) + 1, nan, ERR_SIZE), (0, 0.3, 0), (0, nan, ERR_RANGE)):
        args = list(good)
        args[5], args[6] = steps, eps                                   # steps before epsilon
        assert fn(*args) == code, f"nt_tc_fused_rollout: steps = {steps}"


@pytest.mark.parametrize("dev", DEVICES)
def test_refused_calls_write_nothing(pkg, dev):
    """Both entry points refused for their LAST check (a scalar out of range) and for the overlap, on real buffers: V,
    acc, boards, aux, statistics and status keep every byte."""
    L, B = lib(pkg, dev), 64
    nan = float("nan")
    V, acc = base_on(dev), acc_on(dev)
    boards = t8(dev, NT.K.random_boards(np.random.default_rng(1), B))
    aux = torch.full((B, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    acts = torch.full((B,), 2, dtype=torch.uint8, device=dev)
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    si, sf = torch.full((64,), 7, dtype=torch.int64, device=dev), torch.full((16,), 7.0, dtype=torch.float64, device=dev)
    status = torch.full((1,), 0x777, dtype=torch.int32, device=dev)
    everything = (boards, aux, acts, done, si, sf, status)
    before = [t.clone() for t in everything]
    p = lambda t: t.data_ptr()      # noqa: E731
    inside = p(acc) + V_BYTES       # 256 MiB that lie inside acc, as `weights`
    calls = [
        L.q2048_nt_tc_update(p(V), p(acc), p(boards), p(acts), p(boards), p(done), B, 0.1, nan, p(status), None),
        L.q2048_nt_tc_update(p(V), p(acc), p(boards), p(acts), p(boards), p(done), B, nan, 0.9, p(status), None),
        L.q2048_nt_tc_update(p(V), p(V), p(boards), p(acts), p(boards), p(done), B, 0.1, 0.9, p(status), None),
        L.q2048_nt_tc_update(inside, p(acc), p(boards), p(acts), p(boards), p(done), B, 0.1, 0.9, p(status), None),
        L.q2048_nt_tc_fused_rollout(p(boards), p(aux), p(V), p(acc), B, 3, 0.3, nan, 0.9, 1, 0, 0, p(si), p(sf), p(status), None),
        L.q2048_nt_tc_fused_rollout(p(boards), p(aux), p(V), p(acc), B, 3, 1.5, 0.1, 0.9, 1, 0, 0, p(si), p(sf), p(status), None),
        L.q2048_nt_tc_fused_rollout(p(boards), p(aux), p(V), p(V), B, 3, 0.3, 0.1, 0.9, 1, 0, 0, p(si), p(sf), p(status), None),
        L.q2048_nt_tc_fused_rollout(p(boards), p(aux), inside, p(acc), B, 3, 0.3, 0.1, 0.9, 1, 0, 0, p(si), p(sf), p(status), None),
    ]
    P.sync(dev)
    assert calls == [ERR_RANGE] * 8
    for t, b in zip(everything, before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8)), "a refused call wrote"
    NT.assert_base_unwritten(dev, "a refused call wrote the weights")
    assert np.array_equal(bits(acc), bits(base_acc())), "a refused call wrote the accumulators"


# ---------------------------------------------------------------------------------------------------------------
# 2. / 3. one update where lanes cannot race; zero history
# ---------------------------------------------------------------------------------------------------------------
def transitions(O, B):
    """test_ntuple's transitions for B lanes that cannot race, with its done flags; built once per B"""
    if ("trans", B) not in _SHARED:
        rng = np.random.default_rng(300 + B)
        s, actions, s2 = NT.nonracing_transitions(O, rng, B)
        assert len(s) == B, f"only {len(s)} lanes that cannot race among {NT.MAX_CANDIDATES} candidates"
        assert not NT.conflicts(NT.entry_sets_many(O, s, actions.astype(np.int64), s2))
        _SHARED[("trans", B)] = (s, actions, s2, (rng.random(B) < 0.3).astype(np.uint8))
    return _SHARED[("trans", B)]


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [65, 257, 1000])
def test_update_where_lanes_cannot_race(pkg, O, dev, B):
    """No lane reads or writes an entry another lane writes (acc is read and written only at a lane's write set, so the
    disjointness of test_ntuple's transitions covers it): the sequential model is the specification.  All 768 MiB are
    compared.  Bad actions, illegal actions, done = 1 and a dead s' are all present; the entries visited hold all four
    kinds of history; as many pairs change as there are distinct written entries; and a weight at rate 0 keeps its bits
    while its pair moves."""
    L, V, H = lib(pkg, dev), base_values(), base_acc()
    s, actions, s2, done = transitions(O, B)
    lr, gamma = 0.1, 0.97
    want_v, want_h, want_status, written, es = model_tc_update(O, V, H, s, actions, s2, done, lr, gamma)
    wrote = written[:, 0, 0] >= 0
    bad = actions > 3
    dead = (s2 == P.DEAD.numpy()).all(axis=1)
    assert bad.any() and (~wrote & ~bad).any() and want_status == BAD_ACTION
    assert (wrote & (done == 1)).any() and (wrote & dead & (done == 0)).any() and (wrote & ~dead & (done == 0)).any()
    ids = np.unique(ids_of(written))
    cats = categories(H, ids)
    print(f"B = {B}: {len(ids)} distinct entries written; history A = 0 / |E| = A / between / E = 0: {cats}")
    assert min(cats) > 0 and sum(cats) == len(ids)
    assert (es[wrote] != 0).all()
    assert changed_pairs(want_h, H) == len(ids), "as many pairs change as distinct entries are written"
    still = ids[(H.reshape(-1, 2)[ids, 1] > 0) & (H.reshape(-1, 2)[ids, 0] == 0)]        # rate 0
    assert len(still) and np.array_equal(bits(want_v).ravel()[still], bits(V).ravel()[still])
    assert (bits(want_h).reshape(-1, 2)[still] != bits(H).reshape(-1, 2)[still]).any(axis=1).all()
    moved = np.count_nonzero(bits(want_v) != bits(V))
    assert len(ids) - len(still) >= moved > len(ids) // 2
    plain, _, _ = NT.model_update(O, V, s, actions, s2, done, lr, gamma)
    assert not np.array_equal(bits(plain), bits(want_v)), "the rates do not show"
    del plain

    weights, acc = t32(dev, V), t32(dev, H)
    assert tc_update(L, dev, weights, acc, s, actions, s2, done, lr, gamma) == want_status
    assert_same_bits(weights, want_v, f"V, B = {B}")
    assert_same_bits(acc, want_h, f"acc, B = {B}")
    assert_coherent(acc, f"B = {B}")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [65, 257, 1000])
def test_zero_history_is_the_plain_step(pkg, O, dev, B):
    """Property (a): on acc = 0 every rate is 1 and V after q2048_nt_tc_update is bit for bit V after q2048_nt_update,
    both run here; every written pair is {e, |e|} with the model's e, everything else of acc stays zero."""
    L, V = lib(pkg, dev), base_values()
    s, actions, s2, done = transitions(O, B)
    lr, gamma = 0.1, 0.97
    zero = np.zeros((4, NIDX, 2), F32)
    _, want_h, want_status, written, es = model_tc_update(O, V, zero, s, actions, s2, done, lr, gamma)
    del zero
    plain, status = t32(dev, V), torch.zeros(1, dtype=torch.int32, device=dev)
    ts, ts2, ta, td = t8(dev, s), t8(dev, s2), t8(dev, actions), t8(dev, done)
    assert L.q2048_nt_update(plain.data_ptr(), ts.data_ptr(), ta.data_ptr(), ts2.data_ptr(), td.data_ptr(), B, lr, gamma,
                             status.data_ptr(), None) == 0
    weights, acc = t32(dev, V), torch.zeros((4, NIDX, 2), dtype=torch.float32, device=dev)
    assert tc_update(L, dev, weights, acc, s, actions, s2, done, lr, gamma) == want_status == int(status.item())
    assert_same_bits(weights, plain, f"one step from no history is the plain step, B = {B}")
    assert not np.array_equal(bits(weights), bits(V))
    got = acc.cpu().numpy()
    assert_same_bits(got, want_h, f"acc, B = {B}")
    flat = got.reshape(-1, 2)
    for i in np.flatnonzero(written[:, 0, 0] >= 0):
        mine = (written[i] + (np.arange(4) * NIDX)[:, None]).ravel()
        assert es[i] != 0 and (bits(flat[mine, 0]) == bits(es[i])).all() and (bits(flat[mine, 1]) == bits(np.abs(es[i]))).all()
    assert np.count_nonzero(flat[:, 1]) == len(np.unique(ids_of(written)))


# ---------------------------------------------------------------------------------------------------------------
# 4. boards with a symmetry
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", DEVICES)
def test_symmetric_boards(pkg, O, dev):
    """The three afterstates with one mirror of test_ntuple.test_symmetric_boards (16 distinct entries among 32 each)
    and the empty board as s (no write), one lane per call: each distinct weight moves by its d_i ONCE and each
    distinct pair by {e, |e|} ONCE, not once per occurrence; everything else of the 768 MiB is unchanged."""
    L, V, H = lib(pkg, dev), base_values(), base_acc()
    cases = NT.symmetric_cases()
    assert [n for _, _, n in cases] == [4, 4, 8, 16, 16]
    s = np.stack([
        np.array([5, 6, 6, 5, 7, 8, 8, 7, 0, 0, 0, 0, 9, 10, 10, 9], np.uint8),          # up -> mirrored left-right
        cases[1][1],                                                                      # left -> mirrored top-bottom
        np.array([11, 12, 13, 14, 0, 12, 15, 11, 0, 13, 0, 11, 0, 0, 14, 0], np.uint8),   # left -> its own transpose
        np.zeros(16, np.uint8),                                                           # the empty board: nothing moves
    ])
    actions = np.array([1, 0, 0, 2], np.uint8)
    x = [O.move(s[i], int(actions[i])) for i in range(4)]
    assert [bool(r[2]) for r in x] == [True, True, True, False]
    rng = np.random.default_rng(41)
    s2 = np.stack([AV.spawned(rng, x[i][0]) for i in range(4)])
    done = np.zeros(4, np.uint8)
    lr, gamma = 0.1, 0.97
    want_v, want_h, _, written, es = model_tc_update(O, V, H, s, actions, s2, done, lr, gamma)
    assert (written[3] == -1).all()
    pp = np.arange(4)[:, None]
    distinct = [len(np.unique(ids_of(written[k:k + 1]))) for k in range(3)]
    assert distinct == [16, 16, 16] and len(np.unique(ids_of(written))) == 48, "the three afterstates share no entry"
    assert changed_pairs(want_h, H) == 48, "each distinct pair moves, once"
    for k in range(3):                                                   # ... by e and d_i, not by a multiple
        err = gamma * float(NT.model_best(*NT.model_eval(O, V, s2[k:k + 1])[:2])[0]) - float(NT.model_v(V, x[k][0][None])[0])
        e, idx = F32(err), written[k]
        assert e == es[k] and e != 0
        h = H[pp, idx]
        d = (((lr * 0.03125) * err) * model_rate(h[..., 0], h[..., 1]).astype(np.float64)).astype(F32)
        assert np.array_equal(bits(want_v[pp, idx]), bits(V[pp, idx] + d))
        assert np.array_equal(bits(want_h[pp, idx, 0]), bits(h[..., 0] + e))
        assert np.array_equal(bits(want_h[pp, idx, 1]), bits(h[..., 1] + np.abs(e)))
    weights, acc = t32(dev, V), t32(dev, H)
    for k in range(4):
        assert tc_update(L, dev, weights, acc, s[k:k + 1], actions[k:k + 1], s2[k:k + 1], done[k:k + 1], lr, gamma) == 0
    assert_same_bits(weights, want_v, "V on symmetric afterstates")
    assert_same_bits(acc, want_h, "acc on symmetric afterstates")


# ---------------------------------------------------------------------------------------------------------------
# 5. - 8. the fused learner
# ---------------------------------------------------------------------------------------------------------------
def loaded_agent(pkg, dev, V, H, **kw):
    agent = make_agent(pkg, dev, **kw)
    agent.weights.copy_(t32("cpu", V))
    if H is not None:
        agent.coherence.copy_(t32("cpu", H))
    return agent


def fused_run(pkg, dev, V, H, B, launches, seed, id0, eps, lr, gamma, boards=None, coherence=True):
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    agent = loaded_agent(pkg, dev, V, H if coherence else None, eps=eps, lr=lr, gamma=gamma, seed=seed, id0=id0,
                         coherence=coherence)
    if boards is not None:
        env.boards.copy_(torch.from_numpy(boards))
    for k in launches:
        agent.fused_rollout(env, k)
    assert agent.check_status() == 0
    return env, agent


def four_call_run(pkg, O, dev, V, H, B, steps, seed, id0, eps, lr, gamma, boards=None, learn=True):
    """choose_action -> env.step -> update_q_value (q2048_nt_tc_update, pinned to the model above) -> env.reset(done),
    `steps` times, with the statistics the fused learner counts (test_ntuple.four_call_run's).
    -> (env, agent, statistics, transitions)"""
    env = pkg.BatchedGame2048Env(B, seed=seed, env_id0=id0, device=dev)
    agent = loaded_agent(pkg, dev, V, H, eps=eps, lr=lr, gamma=gamma, seed=seed, id0=id0)
    if boards is not None:
        env.boards.copy_(torch.from_numpy(boards))
    thr = 0 if eps <= 0.0 else int(np.ceil(eps * 4294967296.0))
    st = {"steps": 0, "episodes": 0, "valid_moves": 0, "explored": 0, "score_sum": 0}
    trans = []
    for t in range(steps):
        s = env.boards.cpu().numpy().copy()
        has_move = env.legal_moves().cpu().numpy() != 0
        actions = agent.choose_action(env.boards)
        tb = env.boards.clone()
        s2, reward, done, _ = env.step(actions)
        s2n, a, d = s2.cpu().numpy().copy(), actions.cpu().numpy(), done.cpu().numpy().copy()
        st["steps"] += B
        st["episodes"] += int(d.sum())
        st["valid_moves"] += int((s != s2n).any(axis=1).sum())
        st["score_sum"] += int(env.score.cpu().numpy()[d].sum())
        if eps > 0.0:
            st["explored"] += sum(int(O.draws(seed, id0 + i, t)[0]) < thr and bool(has_move[i]) for i in range(B))
        assert np.array_equal(tb.cpu().numpy(), s)
        if learn:
            agent.update_q_value(tb, actions, reward, s2, done)
        trans.append((s, a, s2n, d.astype(np.uint8)))
        env.reset(done)
    assert agent.check_status() == 0
    return env, agent, st, trans


@pytest.mark.parametrize("dev", DEVICES)
def test_fused_one_lane_many_steps(pkg, O, dev):
    """B = 1, lr 0.1, gamma 0.97, epsilon 0.3, 300 steps in launches of 1, 63 and 236, from the base values and the base
    history: one lane is the sequential learner, so the result is the four-call loop with q2048_nt_tc_update -- boards,
    aux, statistics and all 768 MiB bit for bit.  The first learning step of the run is also checked against the model."""
    seed, id0, eps, lr, gamma, cuts = 5, 77, 0.3, 0.1, 0.97, (1, 63, 236)
    V, H = base_values(), base_acc()
    env_loop, loop, st_loop, trans = four_call_run(pkg, O, dev, V, H, 1, sum(cuts), seed, id0, eps, lr, gamma)
    assert st_loop["episodes"] > 0 and 0 < st_loop["explored"] < sum(cuts)
    env, agent = fused_run(pkg, dev, V, H, 1, cuts, seed, id0, eps, lr, gamma)
    LT.assert_same_run(env, agent, env_loop, st_loop, "B = 1")
    assert_same_bits(agent.weights, loop.weights, "V after 300 sequential steps")
    assert_same_bits(agent.coherence, loop.coherence, "acc after 300 sequential steps")
    got_h = agent.coherence.cpu().numpy()
    assert changed_pairs(got_h, H) > 300
    assert_coherent(got_h, "B = 1")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("B", [65, 257, 1000])
def test_fused_one_learning_step(pkg, O, dev, B):
    """One learning step (lr 0.1, gamma 0.97, epsilon 0.3) on test_ntuple's boards whose lanes cannot race:
    model_tc_update on the transitions of the four-call loop is the specification.  All 768 MiB bit for bit; boards, aux
    and statistics equal."""
    seed, id0, eps, lr, gamma = 23, 4000, 0.3, 0.1, 0.97
    V, H = base_values(), base_acc()
    boards = NT.nonracing_boards(pkg, O, V, B, seed, id0, eps)
    env_loop, _, st_loop, trans = four_call_run(pkg, O, dev, V, H, B, 1, seed, id0, eps, lr, gamma, boards=boards, learn=False)
    s, a, s2, d = trans[0]
    want_v, want_h, status, written, _ = model_tc_update(O, V, H, s, a, s2, d, lr, gamma)
    wrote = int((written[:, 0, 0] >= 0).sum())
    assert status == 0 and wrote > B // 2 and 0 < st_loop["explored"] < B
    assert min(categories(H, ids_of(written))) > 0
    assert changed_pairs(want_h, H) == len(np.unique(ids_of(written))) >= 16 * wrote
    env, agent = fused_run(pkg, dev, V, H, B, (1,), seed, id0, eps, lr, gamma, boards=boards)
    LT.assert_same_run(env, agent, env_loop, st_loop, f"B = {B}")
    assert_same_bits(agent.weights, want_v, f"V, B = {B}")
    assert_same_bits(agent.coherence, want_h, f"acc, B = {B}")


@pytest.mark.parametrize("dev", DEVICES)
def test_lr_zero_accumulates_only(pkg, O, dev):
    """lr = 0, B = 1000, 50 steps in launches of 1 + 49: V is bit-identical (gathered + 0.0; the base holds no -0.0),
    boards, aux and statistics are those of q2048_nt_fused_rollout at lr = 0 on the same seed, and acc has changed and
    is still coherent."""
    B, cuts, seed, id0, eps, gamma = 1000, (1, 49), 17, 1000, 0.3, 0.97
    V, H = base_values(), base_acc()
    env_p, plain = fused_run(pkg, dev, V, None, B, cuts, seed, id0, eps, 0.0, gamma, coherence=False)
    assert plain.coherence is None
    env, agent = fused_run(pkg, dev, V, H, B, cuts, seed, id0, eps, 0.0, gamma)
    P.sync(dev)
    assert torch.equal(env.boards, env_p.boards) and torch.equal(env.aux, env_p.aux)
    assert torch.equal(agent.stats_i, plain.stats_i) and torch.equal(agent.stats_f, plain.stats_f)
    st = agent.stats()
    assert st["steps"] == B * sum(cuts) and st["episodes"] > 0 and 0 < st["explored"] < st["steps"]
    assert_same_bits(agent.weights, V, "lr = 0 wrote V")
    assert_same_bits(plain.weights, V, "the plain learner at lr = 0 wrote V")
    got_h = agent.coherence.cpu().numpy()
    assert changed_pairs(got_h, H) > B
    assert_coherent(got_h, "lr = 0")


@pytest.mark.parametrize("dev", DEVICES)
def test_racing_at_65536_boards_properties(pkg, O, dev):
    """65,536 lanes, epsilon = 1, 4 steps in launches of 1 + 3, from zeros: an exploring choice does not read the
    values, so the trajectories equal those of the four-call loop whatever the racing writes do.  Only entries some
    lane's afterstate visited change, in V and in acc; every pair is finite with A >= 0 and |E| <= A EXACTLY (property
    (b): a torn or half-updated pair would break it); every step, valid move and exploration is counted."""
    B, steps, seed = 65536, 4, 31
    env = pkg.BatchedGame2048Env(B, seed=seed, device=dev)
    agent = make_agent(pkg, dev, eps=1.0, lr=0.05, gamma=0.9, seed=seed, id0=0)
    agent.fused_rollout(env, 1)
    agent.fused_rollout(env, steps - 1)
    loop_env = pkg.BatchedGame2048Env(B, seed=seed, device=dev)
    loop = make_agent(pkg, dev, eps=1.0, lr=0.05, gamma=0.9, seed=seed, id0=0, coherence=False)
    loop.weights = agent.weights                           # an exploring choice reads none
    visited = np.zeros(4 * NIDX, bool)
    valid = explored = 0
    for _ in range(steps):
        s = loop_env.boards.cpu().numpy().copy()
        explored += int((loop_env.legal_moves() != 0).sum())
        a = loop.choose_action(loop_env.boards)
        _, _, done, _ = loop_env.step(a)
        a = a.cpu().numpy()
        moved, _, legal = NT.model_moves(O, s)
        took = legal[np.arange(B), a]
        valid += int(took.sum())
        visited[NT.entry_ids(moved[np.arange(B), a][took]).ravel()] = True
        loop_env.reset(done)
    P.sync(dev)
    assert torch.equal(env.boards, loop_env.boards) and torch.equal(env.aux, loop_env.aux)
    st = agent.stats()
    assert st["steps"] == B * steps and st["valid_moves"] == valid and st["explored"] == explored == valid
    v = agent.weights.cpu().numpy().ravel()
    changed = np.flatnonzero(v)
    assert np.isfinite(v[changed]).all() and np.abs(v[changed]).max() < 1e4
    assert len(changed) and visited[changed].all(), "an entry no lane visited was written"
    assert len(changed) > int(visited.sum()) // 2 and agent.check_status() == 0
    h = agent.coherence.cpu().numpy()
    assert_coherent(h, "65,536 racing lanes")
    touched = np.flatnonzero((bits(h) != 0).any(axis=-1).ravel())
    assert len(touched) and visited[touched].all(), "a pair no lane visited was written"
    assert len(touched) > int(visited.sum()) // 2
    cs = agent.coherence_summary()
    assert cs["visited"] == np.count_nonzero(h[..., 1] > 0) / (4 * NIDX) and 0.0 < cs["mean_rate"] <= 1.0


# ---------------------------------------------------------------------------------------------------------------
# 9. the Python surface and the checkpoint
# ---------------------------------------------------------------------------------------------------------------
def tc_state(agent, env):
    return P.learner_state(agent, env) + (P.bits(agent.coherence),)


@pytest.mark.parametrize("dev", DEVICES)
def test_checkpoint_resumes_the_run(pkg, dev):
    """120 steps, a checkpoint, a fresh agent and env, 80 more == 200 uninterrupted steps at B = 1 in all of V and acc,
    boards, aux, statistics, counters and epsilon; the file keeps the family's kind and adds "coherence"."""
    def run(cuts):
        env = P.make_env(pkg, dev, 1)
        agent = make_agent(pkg, dev, eps=0.9, epochs=10)
        for k, steps in enumerate(cuts):
            agent.fused_rollout(env, steps)
            agent.decay_exploration(k)
            yield env, agent

    for env, agent in run([120, 80]):
        pass
    whole = tc_state(agent, env)
    del agent
    (env1, agent1), = run([120])
    sd, esd = agent1.state_dict(), env1.state_dict()
    assert sd["kind"] == "ntuple6_afterstate" and sd["coherence"].device.type == "cpu"
    assert sd["coherence"].dtype == torch.float32 and tuple(sd["coherence"].shape) == (4, NIDX, 2)
    assert bool(sd["coherence"].any()) and "coherence" not in make_agent(pkg, dev, coherence=False).state_dict()
    env2 = P.make_env(pkg, dev, 1, seed=1, id0=2)
    agent2 = make_agent(pkg, dev, eps=0.1, seed=1, id0=2, epochs=10)
    agent2.load_state_dict(sd)
    env2.load_state_dict(esd)
    P.assert_same_state(tc_state(agent2, env2), tc_state(agent1, env1))      # the round trip
    del agent1, sd
    agent2.fused_rollout(env2, 80)
    agent2.decay_exploration(1)
    P.sync(dev)
    P.assert_same_state(tc_state(agent2, env2), whole)


@pytest.mark.parametrize("dev", DEVICES)
def test_loading_in_every_combination(pkg, dev):
    """plain <- TC file: the accumulators are ignored, and the plain agent plays the games of the TC agent's weights;
    TC <- plain file: same values, accumulators back to zero; TC <- TC file with a broken accumulator (A < 0, |E| > A,
    a NaN, an infinity, wrong shape, wrong dtype, not a tensor): refused before anything is written."""
    env, tc = P.make_env(pkg, dev, 64), make_agent(pkg, dev)
    tc.fused_rollout(env, 20)
    tc_sd = tc.state_dict()
    plain = make_agent(pkg, dev, coherence=False, seed=9, id0=9)
    plain.load_state_dict(tc_sd)
    assert plain.coherence is None and "coherence" not in plain.state_dict()
    assert torch.equal(P.bits(plain.weights), P.bits(tc.weights)) and plain.ctr == tc.ctr
    games = []
    for player in (plain, tc):
        e = P.make_env(pkg, dev, 96, seed=3, id0=500)
        player.play_rollout(e, 40)
        player.play_rollout(e, 160)
        P.sync(dev)
        games.append((e.boards.cpu(), e.aux.cpu(), player.play_stats()))
    assert torch.equal(games[0][0], games[1][0]) and torch.equal(games[0][1], games[1][1]) and games[0][2] == games[1][2]
    assert games[0][2]["steps"] == 96 * 200 and games[0][2]["episodes"] > 0
    with pytest.raises(ValueError):
        plain.coherence_summary()

    plain_sd = dict(plain.state_dict(), ctr=555)
    other = make_agent(pkg, dev, seed=9, id0=9)
    other.coherence.fill_(1.0)
    other.load_state_dict(plain_sd)
    assert other.ctr == 555 and torch.equal(P.bits(other.weights), P.bits(tc.weights))
    assert not bool(other.coherence.any()), "a plain file restarts the accumulators at zero"
    assert other.coherence_summary() == {"visited": 0.0, "mean_rate": 1.0}
    del other, plain, plain_sd

    before = tc_state(tc, env)
    h = tc_sd["coherence"]
    p, i = [int(x) for x in torch.nonzero(h[..., 1] > 0)[0]]
    marked = dict(tc_sd, ctr=999, stats_i=tc_sd["stats_i"] + 1)
    keep = h[p, i].clone()
    for pair in ((0.5, -1.0), (-0.0, -0.25), (2.0, 1.0), (-2.0, 1.0), (float("nan"), 1.0), (0.0, float("nan")),
                 (float("inf"), float("inf")), (0.0, float("inf"))):
        h[p, i] = torch.tensor(pair)
        with pytest.raises(ValueError, match="coherence"):
            tc.load_state_dict(marked)
        h[p, i] = keep
    for wrong in (h[:, :4096], h[..., 0], h.reshape(4, 2, NIDX), h.view(torch.int32), h.numpy(), h[:2]):
        with pytest.raises(ValueError, match="coherence"):
            tc.load_state_dict(dict(marked, coherence=wrong))
    with pytest.raises(ValueError):
        tc.load_state_dict(dict(marked, weights=marked["weights"][:2]))     # a good accumulator, the rest wrong
    P.sync(dev)
    P.assert_same_state(tc_state(tc, env), before)
    tc.load_state_dict(marked)
    assert tc.ctr == 999 and torch.equal(P.bits(tc.coherence), P.bits(h))


@pytest.mark.parametrize("dev", DEVICES)
def test_python_surface(pkg, O, dev):
    """`update_q_value` of a coherence agent is q2048_nt_tc_update (and ignores its reward argument), what only reads V
    is the plain agent's, and `coherence_summary` is the share of pairs with A > 0 and the mean of min(|E| / A, 1) over
    them."""
    V, H = base_values(), base_acc()
    agent = make_agent(pkg, dev, lr=0.1)
    agent.weights, agent.coherence = t32(dev, V), t32(dev, H)
    boards = AV.midgame(O)[0][:300]
    q, _, _ = NT.model_eval(O, V, boards, tuple(m[:300] for m in AV.midgame(O)[1]))
    assert_same_bits(agent.values(t8(dev, boards)), NT.model_v(V, boards), "values")
    assert_same_bits(agent.q_values(t8(dev, boards)), q, "q_values")
    cs = agent.coherence_summary()
    E, A = H[..., 0].astype(np.float64), H[..., 1].astype(np.float64)
    seen = A > 0
    assert cs["visited"] == seen.sum() / seen.size and 0.7 < cs["visited"] < 0.8
    assert abs(cs["mean_rate"] - float(model_rate(H[..., 0], H[..., 1])[seen].astype(np.float64).mean())) < 1e-6
    del E, A
    s, actions, s2, _ = transitions(O, 65)
    done = np.zeros(65, np.uint8)
    want_v, want_h, status, _, _ = model_tc_update(O, V, H, s, actions, s2, done, 0.1, 0.95)
    agent.update_q_value(t8(dev, s), actions, np.full(65, 1e6, F32), t8(dev, s2), done)
    assert_same_bits(agent.weights, want_v, "update_q_value: V")
    assert_same_bits(agent.coherence, want_h, "update_q_value: acc")
    assert status == BAD_ACTION
    with pytest.raises(ValueError):
        agent.check_status()                                            # the bad actions among the transitions
    with pytest.raises(ValueError):
        agent.update_q_value(t8(dev, s), actions, np.zeros(64, F32), t8(dev, s2), done)
    with pytest.raises(ValueError):
        agent.fused_rollout(pkg.BatchedGame2048Env(8, 5, dev, agent.seed, agent.env_id0), 1)
    with pytest.raises(ValueError):
        agent.fused_rollout(P.make_env(pkg, dev, 8, "nopenalty"), 1)
