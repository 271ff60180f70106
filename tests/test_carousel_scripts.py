"""Carousel shaping's Python surface -- BatchedNTupleAgent(..., stage_tiles=..., carousel=P) -- its checkpoint in every
combination, and `train.py --carousel P` with --save / --resume: in this process on the CPU twin with one host thread (a learning
run is then sequential and reproducible), and once as subprocesses on the GPU."""
import importlib
import os

import numpy as np
import pytest
import torch

import test_carousel as CA
import test_ntuple as NT
import test_ntuple_scripts as S
import test_ntuple_stages as ST
import test_row_tuple_player as P

script, load, log_rows, same = P.script, P.load, P.log_rows, S.same
DEVICES, NIDX = NT.DEVICES, NT.NIDX


def carousel_agent(pkg, dev, tiles, P_, seed=5, id0=77, eps=0.3, **kw):
    return pkg.BatchedNTupleAgent(100, learning_rate=0.1, discount_factor=0.97, exploration_rate=eps, seed=seed, env_id0=id0,
                                  device=dev, stage_tiles=tiles, carousel=P_, **kw)


def test_constructor_refusals(pkg):
    A = pkg.BatchedNTupleAgent
    with pytest.raises(ValueError, match="stage_tiles"):
        A(10, device="cpu", carousel=16)
    for bad in (-1, 2.0, True, "4", (1 << 32) + 1):
        with pytest.raises(ValueError, match="carousel"):
            A(10, device="cpu", stage_tiles=(2048,), carousel=bad)
    with pytest.raises(ValueError, match="coherence"):
        A(10, device="cpu", stage_tiles=(2048,), carousel=4, coherence=True)
    off = A(10, device="cpu", stage_tiles=(2048,))                   # the default: today's agent
    assert off.carousel == 0 and off.carousel_pool is None and off.carousel_counts is None and off.carousel_fresh is None
    assert "carousel" not in off.state_dict()
    with pytest.raises(ValueError, match="carousel"):
        off.carousel_summary()
    on = A(10, device="cpu", stage_tiles=(8, 64), carousel=5)
    assert tuple(on.carousel_pool.shape) == (3, 5, 32) and on.carousel_pool.dtype == torch.uint8
    assert tuple(on.carousel_counts.shape) == (3,) and on.carousel_counts.dtype == torch.int64 and on.carousel_fresh is None
    assert on.carousel_summary() == {"counts": [0, 0, 0], "valid": [0, 0, 0]}
    assert on.carousel_pool.data_ptr() % 16 == 0


@pytest.mark.parametrize("dev", DEVICES)
def test_checkpoint_round_trip_and_resume_at_one_lane(pkg, dev):
    """B = 1, tiles (8, 64), carousel = 4 from test_carousel's hand-filled pool.  One agent runs 600 + 600 steps; a second
    one runs 600, is saved with its env, and a THIRD, built fresh, loads the file and runs the other 600: weights, boards,
    aux, pool, counts and statistics equal the first agent's bit for bit.  Then the combinations: a carousel agent loads
    a file without a pool (an empty pool; its own is wiped), a plain staged agent ignores a file's pool, another P or S
    is refused before anything is written."""
    tiles, P_ = (8, 64), 4
    pool, counts = CA.one_lane_pool()

    def fresh_pair(weights):
        env = pkg.BatchedGame2048Env(1, seed=5, env_id0=77, device=dev)
        agent = carousel_agent(pkg, dev, tiles, P_)
        if weights is not None:
            agent.weights = weights
            agent.carousel_pool.copy_(torch.from_numpy(pool))
            agent.carousel_counts.copy_(torch.from_numpy(counts.view(np.int64)))
        return env, agent

    env_a, a = fresh_pair(ST.t32(dev, ST.tables(3)))
    a.fused_rollout(env_a, 600)
    a.fused_rollout(env_a, 600)
    env_b, b = fresh_pair(ST.t32(dev, ST.tables(3)))
    b.fused_rollout(env_b, 600)
    sd, env_sd = b.state_dict(), env_b.state_dict()
    assert sd["kind"] == "ntuple6_afterstate" and sd["stage_tiles"] == [8, 64] and set(sd["carousel"]) == {"pool", "counts"}
    assert tuple(sd["carousel"]["pool"].shape) == (3, P_, 32) and sd["carousel"]["counts"].tolist() == b.carousel_summary()["counts"]
    assert sum(sd["carousel"]["counts"].tolist()) > int(counts.sum()), "600 steps commit a record"
    del b, env_b
    env_c, c = fresh_pair(None)
    c.load_state_dict(sd)
    env_c.load_state_dict(env_sd)
    assert torch.equal(c.carousel_pool.cpu(), sd["carousel"]["pool"]) and c.carousel_summary()["counts"] == sd["carousel"]["counts"].tolist()
    c.fused_rollout(env_c, 600)
    P.sync(dev)
    assert torch.equal(env_c.boards.cpu(), env_a.boards.cpu()) and torch.equal(env_c.aux.cpu(), env_a.aux.cpu())
    assert torch.equal(c.carousel_pool, a.carousel_pool) and torch.equal(c.carousel_counts, a.carousel_counts)
    assert torch.equal(c.stats_i, a.stats_i) and c.ctr == a.ctr == 1200
    ST.assert_same_bits(c.weights, a.weights, "save / resume at B = 1")
    del a, env_a
    # a plain staged agent ignores a file's pool; its own file has none
    plain = ST.make_agent(pkg, dev, tiles)
    plain.load_state_dict(sd)
    assert plain.carousel_pool is None and same(plain.weights.cpu(), sd["weights"]) and "carousel" not in plain.state_dict()
    # a carousel agent loads a file without a pool: an empty pool (what it held is wiped), the weights continue
    nopool = {k: v for k, v in sd.items() if k != "carousel"}
    assert bool(c.carousel_counts.any())
    c.load_state_dict(nopool)
    assert not c.carousel_pool.any() and c.carousel_summary() == {"counts": [0, 0, 0], "valid": [0, 0, 0]}
    assert same(c.weights.cpu(), sd["weights"])
    # another P, another S, a pool of another type: refused before anything is written
    c.load_state_dict(sd)
    before_w, before_p, before_c = P.bits(c.weights).clone(), c.carousel_pool.clone(), c.carousel_counts.clone()
    other_p = dict(sd, ctr=999, carousel={"pool": sd["carousel"]["pool"][:, :3].contiguous(), "counts": sd["carousel"]["counts"]})
    other_s = dict(sd, ctr=999, carousel={"pool": sd["carousel"]["pool"][:2].contiguous(), "counts": sd["carousel"]["counts"][:2]})
    other_t = dict(sd, ctr=999, carousel={"pool": sd["carousel"]["pool"].to(torch.int32), "counts": sd["carousel"]["counts"]})
    other_n = dict(sd, ctr=999, carousel={"pool": sd["carousel"]["pool"], "counts": -sd["carousel"]["counts"] - 1})
    for wrong in (other_p, other_s, other_t, other_n, dict(sd, ctr=999, carousel=7)):
        with pytest.raises(ValueError, match="carousel"):
            c.load_state_dict(wrong)
    with pytest.raises(ValueError, match="carousel"):
        carousel_agent(pkg, "cpu", tiles, 5).load_state_dict(sd)
    with pytest.raises(ValueError):
        carousel_agent(pkg, "cpu", (8,), P_).load_state_dict(sd)                       # another S
    with pytest.raises(ValueError):
        c.load_state_dict(dict(sd, ctr=999, weights=sd["weights"][:1]))              # a good pool, bad weights
    assert torch.equal(P.bits(c.weights), before_w) and torch.equal(c.carousel_pool, before_p)
    assert torch.equal(c.carousel_counts, before_c) and c.ctr == sd["ctr"]


def test_train_carousel_save_resume_and_refusals(pkg, tmp_path, monkeypatch):
    """train.main in this process on the CPU twin with one host thread (the run is then sequential and reproducible):
    four epochs at once == two epochs, --save, --resume for the other two, on weights, pool, counts, statistics, boards
    and the log; a staged file without a pool resumes with --carousel; the refusals of the command line are SystemExits
    that name the flag, another P in the file is refused by the agent."""
    train = importlib.import_module("train")
    monkeypatch.setenv("Q2048_HOST_THREADS", "1")
    monkeypatch.chdir(tmp_path)
    base = ["--device", "cpu", "--agent", "ntuple", "--num-envs", "64", "--episodes", "4", "--seed", "4", "--report-every", "1"]
    car = ["--stage-tiles", "16", "--carousel", "32"]
    train.main(base + car + ["--save", "full.pt", "--log", "full.csv"])
    train.main(base + car + ["--stop-epoch", "2", "--save", "part.pt", "--log", "p1.csv"])
    train.main(base + car + ["--resume", "part.pt", "--save", "resumed.pt", "--log", "p2.csv"])
    a, b = load(tmp_path, "full.pt"), load(tmp_path, "resumed.pt")
    assert a["stage_tiles"] == [16] and tuple(a["carousel"]["pool"].shape) == (2, 32, 32)
    counts = a["carousel"]["counts"].tolist()
    assert counts[0] == 0 and counts[1] > 32, counts
    assert b["train"]["epoch"] == 4 and same(a["weights"], b["weights"]) and a["ctr"] == b["ctr"]
    assert torch.equal(a["carousel"]["pool"], b["carousel"]["pool"]) and torch.equal(a["carousel"]["counts"], b["carousel"]["counts"])
    assert torch.equal(a["stats_i"], b["stats_i"]) and torch.equal(a["env"]["boards"], b["env"]["boards"])
    assert log_rows(tmp_path, "p1.csv") + log_rows(tmp_path, "p2.csv") == log_rows(tmp_path, "full.csv")
    # a file without a pool resumes with --carousel: an empty pool that the run then fills
    nopool = {k: v for k, v in load(tmp_path, "part.pt").items() if k != "carousel"}
    torch.save(nopool, tmp_path / "nopool.pt")
    del a, b, nopool
    train.main(base + car + ["--resume", "nopool.pt", "--save", "into.pt", "--log", "i.csv"])
    assert load(tmp_path, "into.pt")["carousel"]["counts"].tolist()[1] > 0
    # the refusals
    for extra, word in ((["--carousel", "32"], "--carousel applies with --stage-tiles"),
                        (["--agent", "afterstate", "--carousel", "32"], "--carousel applies with --stage-tiles"),
                        (["--stage-tiles", "16", "--carousel", "0"], "--carousel"),
                        (["--stage-tiles", "16", "--carousel", "-3"], "--carousel")):
        with pytest.raises(SystemExit, match=word):
            train.main(base + extra + ["--save", "never.pt", "--log", "bad.csv"])
    with pytest.raises(ValueError, match="carousel"):
        train.main(base + ["--stage-tiles", "16", "--carousel", "8", "--resume", "full.pt", "--save", "never.pt", "--log", "bad.csv"])
    assert not os.path.exists(tmp_path / "never.pt")


@pytest.mark.gpu
def test_train_carousel_on_the_device(pkg, tmp_path):
    t = script(tmp_path, "cuda", "train.py", "--agent", "ntuple", "--stage-tiles", "32,128", "--carousel", "256", "--num-envs",
               "1024", "--episodes", "3", "--report-every", "1", "--save", "g.pt", "--log", "g.csv")
    assert t.returncode == 0, t.stderr[-2000:]
    g = load(tmp_path, "g.pt")
    counts = g["carousel"]["counts"].tolist()
    assert g["stage_tiles"] == [32, 128] and counts[0] == 0 and counts[1] > 256 and counts[2] > 0, counts
    pool = g["carousel"]["pool"].numpy()
    for k in (1, 2):
        n = min(counts[k], 256)
        assert (ST.model_stage(pool[k, :n, :16], (5, 7)) == k).all() and not pool[k, :n, 24:].any()
    r = script(tmp_path, "cuda", "train.py", "--agent", "ntuple", "--stage-tiles", "32,128", "--carousel", "256", "--num-envs",
               "1024", "--episodes", "4", "--report-every", "1", "--resume", "g.pt", "--save", "h.pt", "--log", "h.csv")
    assert r.returncode == 0, r.stderr[-2000:]
    h = load(tmp_path, "h.pt")
    assert all(x >= y for x, y in zip(h["carousel"]["counts"].tolist(), counts)) and h["train"]["epoch"] == 4
