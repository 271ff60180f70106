"""The staged 6-tuple network's Python surface, its checkpoint in every combination, and the scripts:
`train.py --agent ntuple --stage-tiles ... --save / --resume / --promote-every`, a plain file split by
`--resume PLAIN --stage-tiles ...`, and `evaluate.py` on a staged file in the loop form, with `--fused` and with
`--search` at both depths.  The scripts run as subprocesses on the CPU twin with one host thread (a learning run is then
sequential and reproducible), and once on the GPU.  A staged file of two stages is 512 MiB: files are removed where the
test no longer needs them."""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import test_ntuple as NT
import test_ntuple_scripts as S
import test_ntuple_stages as ST
import test_row_tuple_player as P

script, load, log_rows, same, last_json, KEYS = P.script, P.load, P.log_rows, S.same, S.last_json, S.KEYS
DEVICES, NIDX, bits = NT.DEVICES, NT.NIDX, NT.bits


@pytest.mark.parametrize("dev", DEVICES)
def test_python_surface_and_checkpoint(pkg, O, dev):
    """The constructor's checks; every method of a staged agent against the staged model; the checkpoint: staged into
    staged (bit for bit), a plain file into a staged agent (stage 0 = the file, the rest promoted: every stage equals the
    file), and the refusals -- other tiles, a staged file into a plain agent, every crossing of kinds -- which write
    nothing."""
    A = pkg.BatchedNTupleAgent
    for bad in ((3,), (0,), (2048, 2048), (4096, 2048), (65536,), (2, 4, 8, 16, 32, 64, 128, 256), (2.0,), (True,)):
        with pytest.raises(ValueError):
            A(10, device=dev, stage_tiles=bad)
    with pytest.raises(ValueError, match="coherence"):
        A(10, device=dev, stage_tiles=(2048,), coherence=True)
    plain = NT.make_agent(pkg, dev)
    assert plain.stage_tiles == () and tuple(plain.weights.shape) == (4, NIDX) and "stage_tiles" not in plain.state_dict()
    Vs, thr = ST.tables(2), (8,)
    agent = ST.make_agent(pkg, dev, (256,), lr=0.1, gamma=0.95, weights=ST.t32(dev, Vs))
    assert agent._stages == 8 and tuple(agent.weights.shape) == (2, 4, NIDX)
    boards = ST.capped_boards(np.random.default_rng(7), 300)
    tb = ST.t8(dev, boards)
    q, legal, _, cstage = ST.model_eval(O, Vs, thr, boards)
    assert len(np.unique(cstage)) == 2
    ST.assert_same_bits(agent.values(tb), ST.model_v(Vs, thr, boards), "values")
    ST.assert_same_bits(agent.q_values(tb), q, "q_values")
    s, actions, s2 = NT.nonracing_transitions(O, np.random.default_rng(365), 65)
    done = np.zeros(65, np.uint8)
    want, status, _, _ = ST.model_update(O, Vs, (15,), s, actions, s2, done, 0.1, 0.95)
    top = ST.make_agent(pkg, dev, (32768,), lr=0.1, gamma=0.95, weights=ST.t32(dev, Vs))
    top.update_q_value(ST.t8(dev, s), actions, np.full(65, 1e6, np.float32), ST.t8(dev, s2), done)
    ST.assert_same_bits(top.weights, want, "update_q_value")
    del top, want

    # staged -> staged
    sd = agent.state_dict()
    assert sd["kind"] == "ntuple6_afterstate" and sd["stage_tiles"] == [256] and tuple(sd["weights"].shape) == (2, 4, NIDX)
    other = ST.make_agent(pkg, dev, (256,))
    other.load_state_dict(sd)
    assert same(other.weights.cpu(), sd["weights"])
    # the refusals: other tiles, more tiles, a staged file into a plain agent; nothing is written
    before = P.bits(other.weights).clone()
    for wrong in ((512,), (256, 1024)):
        with pytest.raises(ValueError, match="stage_tiles"):
            ST.make_agent(pkg, dev, wrong).load_state_dict(sd)
    with pytest.raises(ValueError, match="staged"):
        plain.load_state_dict(sd)
    assert not bool(plain.weights.any()) and plain.ctr == 0
    for kind in ("row_tuple", "line_tuple", "line_afterstate", None):
        crossed = {k: v for k, v in sd.items() if k != "kind"}
        if kind:
            crossed["kind"] = kind
        with pytest.raises(ValueError):
            other.load_state_dict(dict(crossed, ctr=999))
    for o_sd in (pkg.BatchedAfterstateAgent(10, device="cpu").state_dict(), pkg.BatchedRowTupleAgent(10, device="cpu").state_dict()):
        with pytest.raises(ValueError):
            other.load_state_dict(o_sd)
    with pytest.raises(ValueError):
        pkg.BatchedAfterstateAgent(10, device="cpu").load_state_dict(sd)
    with pytest.raises(ValueError):
        other.load_state_dict(dict(sd, weights=sd["weights"][:1]))
    assert torch.equal(P.bits(other.weights), before) and other.ctr == sd["ctr"]
    del other, before, sd
    # plain -> staged: stage 0, zeros, promotion; every stage equals the file (the base values hold no zero bits ...
    # but a trained file does: those entries stay zero in every stage, which is the file's value too)
    plain.weights = NT.t32(dev, NT.base_values())
    plain.weights[0, :1000] = 0.0
    psd = dict(plain.state_dict(), ctr=41)
    three = ST.make_agent(pkg, dev, (8, 64), weights=ST.t32(dev, ST.tables(3)))
    three.load_state_dict(psd)
    assert three.ctr == 41 and all(same(three.weights[k].cpu(), psd["weights"]) for k in range(3))
    assert three.promote() == [0, 0]


def test_train_save_resume_split_and_evaluate(pkg, tmp_path):
    train = ("train.py", "--agent", "ntuple", "--num-envs", "64", "--episodes", "6", "--seed", "4", "--report-every", "1")
    run = lambda *a: script(tmp_path, "cpu", *train, *a)   # noqa: E731
    # thresholds the small run reaches: 16 and 64
    staged = ("--stage-tiles", "16,64")
    full = run(*staged, "--save", "full.pt", "--log", "full.csv", "--eval-every", "3", "--eval-envs", "64", "--eval-log", "E.jsonl")
    assert full.returncode == 0, full.stderr[-2000:]
    assert len([ln for ln in full.stdout.splitlines() if "promoted" in ln]) == 6           # --promote-every defaults to 1
    assert [json.loads(ln)["epoch"] for ln in open(tmp_path / "E.jsonl").read().splitlines()] == [3, 6]
    part = run(*staged, "--stop-epoch", "3", "--save", "part.pt", "--log", "p1.csv")
    assert part.returncode == 0, part.stderr[-2000:]
    rest = run(*staged, "--resume", "part.pt", "--save", "resumed.pt", "--log", "p2.csv")
    assert rest.returncode == 0, rest.stderr[-2000:]
    a = load(tmp_path, "full.pt")
    assert a["kind"] == "ntuple6_afterstate" and a["stage_tiles"] == [16, 64] and tuple(a["weights"].shape) == (3, 4, 1 << 24)
    assert all(bool(a["weights"][k].any()) for k in range(3)), "the run reaches every stage"
    assert not same(a["weights"][0], a["weights"][1]) and not same(a["weights"][1], a["weights"][2])
    b = load(tmp_path, "resumed.pt")
    assert b["train"]["epoch"] == 6 and same(a["weights"], b["weights"]) and a["ctr"] == b["ctr"]
    assert torch.equal(a["stats_i"], b["stats_i"]) and torch.equal(a["env"]["boards"], b["env"]["boards"])
    del a, b
    os.remove(tmp_path / "resumed.pt")
    os.remove(tmp_path / "part.pt")
    assert log_rows(tmp_path, "p1.csv") + log_rows(tmp_path, "p2.csv") == log_rows(tmp_path, "full.csv")
    # the refusals of the command line, and of a file with other tiles
    for extra, word in ((("--stage-tiles", "16", "--coherence"), "--coherence"), (("--stage-tiles", "24"), "--stage-tiles"),
                        (("--stage-tiles", "64,16"), "--stage-tiles"), (("--promote-every", "2"), "--promote-every"),
                        (("--stage-tiles", "16", "--resume", "full.pt"), "stage_tiles"), (("--resume", "full.pt"), "staged")):
        bad = run(*extra, "--save", "never.pt", "--log", "bad.csv")
        assert bad.returncode != 0 and word in bad.stderr, (extra, bad.stderr[-500:])
    bad = script(tmp_path, "cpu", "train.py", "--agent", "afterstate", "--num-envs", "64", "--episodes", "2", "--stage-tiles", "16")
    assert bad.returncode != 0 and "--stage-tiles applies to --agent ntuple" in bad.stderr
    assert not os.path.exists(tmp_path / "never.pt")
    # evaluate.py reads the setting from the file: the loop form, --fused, --search at both depths
    common = ("evaluate.py", "--model", "full.pt", "--num-envs", "48", "--episodes", "1", "--steps-per-launch", "16", "--seed", "5")
    x, y = (script(tmp_path, "cpu", *common, *f) for f in ((), ("--fused",)))
    assert x.returncode == 0 and y.returncode == 0, x.stderr[-2000:] + y.stderr[-2000:]
    x, y = last_json(x), last_json(y)
    assert x["agent"] == y["agent"] == "ntuple" and x["stage_tiles"] == y["stage_tiles"] == [16, 64] and y["fused"] is True
    for key in KEYS:
        assert x[key] == y[key], key
    few = ("evaluate.py", "--model", "full.pt", "--num-envs", "3", "--episodes", "1", "--steps-per-launch", "16", "--seed", "5",
           "--fused", "--search")
    z1, z2 = script(tmp_path, "cpu", *few), script(tmp_path, "cpu", *few, "--search-depth", "2")
    assert z1.returncode == 0 and z2.returncode == 0, z1.stderr[-2000:] + z2.stderr[-2000:]
    z1, z2 = last_json(z1), last_json(z2)
    assert (z1["search"], z2["search"]) == (1, 2) and z1["stage_tiles"] == z2["stage_tiles"] == [16, 64] and z2["games"] >= 3
    os.remove(tmp_path / "full.pt")
    # a plain file split by --resume ... --stage-tiles: every stage starts as the file, so at epsilon 0 the split file
    # plays the plain file's games byte for byte (--stop-epoch at the file's epoch: nothing more is learned)
    plain = run("--stop-epoch", "3", "--save", "plain.pt", "--log", "p3.csv")
    assert plain.returncode == 0, plain.stderr[-2000:]
    split = run(*staged, "--resume", "plain.pt", "--stop-epoch", "3", "--save", "split.pt", "--log", "p4.csv")
    assert split.returncode == 0 and "every one of the 3 stages starts as the file" in split.stdout, split.stderr[-2000:]
    p, s = load(tmp_path, "plain.pt"), load(tmp_path, "split.pt")
    assert "stage_tiles" not in p and s["stage_tiles"] == [16, 64] and s["ctr"] == p["ctr"]
    assert all(same(s["weights"][k], p["weights"]) for k in range(3))
    del p, s
    ev = lambda name, *f: script(tmp_path, "cpu", "evaluate.py", "--model", name, "--num-envs", "48", "--episodes", "1",   # noqa: E731
                                 "--steps-per-launch", "16", "--seed", "5", *f)
    for flags in ((), ("--fused",)):
        u, v = ev("plain.pt", *flags), ev("split.pt", *flags)
        assert u.returncode == 0 and v.returncode == 0, u.stderr[-2000:] + v.stderr[-2000:]
        u, v = last_json(u), last_json(v)
        assert u["stage_tiles"] == [] and v["stage_tiles"] == [16, 64]
        for key in KEYS + ("mean_return",):
            assert u[key] == v[key], key
    # ... and the split network then goes on learning
    more = run(*staged, "--resume", "split.pt", "--save", "more.pt", "--log", "p5.csv")
    assert more.returncode == 0, more.stderr[-2000:]
    m = load(tmp_path, "more.pt")
    assert m["train"]["epoch"] == 6 and not same(m["weights"][0], m["weights"][1])


def test_promote_every_cadence(pkg, tmp_path, monkeypatch):
    """train.main in this process on the CPU twin, `promote` counted: once per epoch by default, every second epoch
    with --promote-every 2, never with 0, and never without --stage-tiles."""
    train = importlib.import_module("train")
    calls = []
    real = pkg.BatchedNTupleAgent.promote
    monkeypatch.setattr(pkg.BatchedNTupleAgent, "promote", lambda self: calls.append(self.train_progress["epoch"]) or real(self))
    monkeypatch.setenv("Q2048_HOST_THREADS", "1")
    monkeypatch.chdir(tmp_path)
    base = ["--device", "cpu", "--agent", "ntuple", "--num-envs", "64", "--episodes", "4", "--seed", "4", "--report-every", "1",
            "--log", "c.csv"]
    want = {(): 4, ("--promote-every", "2"): 2, ("--promote-every", "0"): 0, ("--promote-every", "3"): 1}
    for extra, n in want.items():
        calls.clear()
        train.main(base + ["--stage-tiles", "16", *extra])
        assert len(calls) == n, (extra, calls)
    calls.clear()
    train.main(base)
    assert calls == []


@pytest.mark.gpu
def test_the_scripts_on_the_device(pkg, tmp_path):
    t = script(tmp_path, "cuda", "train.py", "--agent", "ntuple", "--stage-tiles", "32,128", "--num-envs", "1024", "--episodes",
               "3", "--report-every", "1", "--save", "g.pt", "--log", "g.csv", "--eval-every", "1", "--eval-envs", "512",
               "--eval-log", "E.jsonl")
    assert t.returncode == 0, t.stderr[-2000:]
    assert [json.loads(ln)["epoch"] for ln in open(tmp_path / "E.jsonl").read().splitlines()] == [1, 2, 3]
    assert "promoted" in t.stdout
    g = load(tmp_path, "g.pt")
    assert g["stage_tiles"] == [32, 128] and all(bool(g["weights"][k].any()) for k in range(3))
    del g
    common = ("evaluate.py", "--model", "g.pt", "--num-envs", "1024", "--episodes", "1")
    x, y, z = (script(tmp_path, "cuda", *common, *f) for f in ((), ("--fused",), ("--fused", "--search")))
    assert x.returncode == 0 and y.returncode == 0 and z.returncode == 0, x.stderr[-2000:] + y.stderr[-2000:] + z.stderr[-2000:]
    x, y, z = last_json(x), last_json(y), last_json(z)
    assert y["stage_tiles"] == [32, 128] and y["fused"] is True and z["search"] == 1 and z["games"] >= 1024
    for key in KEYS:
        assert x[key] == y[key], key
    w = script(tmp_path, "cuda", "evaluate.py", "--model", "g.pt", "--num-envs", "64", "--episodes", "1", "--fused", "--search",
               "--search-depth", "2")
    assert w.returncode == 0 and last_json(w)["search"] == 2, w.stderr[-2000:]
