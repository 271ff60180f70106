"""Temporal-coherence step sizes through the scripts: `train.py --agent ntuple --coherence --save / --resume /
--eval-every` in each direction of resuming (with the refusal and its message), the refusal of `--coherence` with any
other agent, and `evaluate.py --model` on the saved file with and without `--fused --search`.  As subprocesses on the
CPU twin with one host thread (a learning run is then sequential and reproducible).  Small runs: a file with
accumulators is 768 MiB, so files are removed where the test no longer needs them."""
import json
import os

import pytest
import torch

import test_ntuple_scripts as S
import test_row_tuple_player as P

script, load, log_rows, same, last_json = P.script, P.load, P.log_rows, S.same, S.last_json
ACC_SHAPE = (4, 1 << 24, 2)


def test_train_save_resume_and_evaluate(pkg, tmp_path):
    train = ("train.py", "--agent", "ntuple", "--num-envs", "64", "--episodes", "6", "--seed", "4", "--report-every", "1",
             "--alpha", "0.5")
    run = lambda *a: script(tmp_path, "cpu", *train, *a)   # noqa: E731
    full = run("--coherence", "--save", "full.pt", "--log", "full.csv", "--eval-every", "3", "--eval-envs", "128",
               "--eval-log", "E.jsonl")
    assert full.returncode == 0, full.stderr[-2000:]
    part = run("--coherence", "--stop-epoch", "3", "--save", "part.pt", "--log", "p1.csv")
    assert part.returncode == 0, part.stderr[-2000:]
    rest = run("--coherence", "--resume", "part.pt", "--save", "resumed.pt", "--log", "p2.csv")
    assert rest.returncode == 0, rest.stderr[-2000:]
    assert "start at zero" not in rest.stdout
    a = load(tmp_path, "full.pt")
    assert a["kind"] == "ntuple6_afterstate" and a["train"]["epoch"] == 6
    assert tuple(a["coherence"].shape) == ACC_SHAPE and a["coherence"].dtype == torch.float32
    E, A = a["coherence"][..., 0], a["coherence"][..., 1]
    assert bool((A > 0).any()) and bool((E.abs() <= A).all()) and bool(torch.isfinite(a["coherence"]).all())
    del E, A
    # save at epoch 3 + resume == the uninterrupted run: values, accumulators, counters, statistics, boards, the log
    b = load(tmp_path, "resumed.pt")
    assert b["train"]["epoch"] == 6 and same(a["weights"], b["weights"]) and same(a["coherence"], b["coherence"])
    assert a["ctr"] == b["ctr"] and torch.equal(a["stats_i"], b["stats_i"]) and torch.equal(a["stats_f"], b["stats_f"])
    assert torch.equal(a["env"]["boards"], b["env"]["boards"]) and torch.equal(a["env"]["aux"], b["env"]["aux"])
    del b
    os.remove(tmp_path / "resumed.pt")
    assert log_rows(tmp_path, "p1.csv") + log_rows(tmp_path, "p2.csv") == log_rows(tmp_path, "full.csv")
    # the evaluation lines and the final report carry the two numbers of coherence_summary()
    lines = [json.loads(ln) for ln in open(tmp_path / "E.jsonl").read().splitlines()]
    assert [ln["epoch"] for ln in lines] == [3, 6]
    for ln in lines:
        assert 0.0 < ln["coherence_visited"] < 1.0 and 0.0 < ln["coherence_mean_rate"] <= 1.0 and ln["games"] >= 128
    assert lines[0]["coherence_visited"] <= lines[1]["coherence_visited"]
    assert abs(lines[1]["coherence_visited"] - float((a["coherence"][..., 1] > 0).sum()) / (4 << 24)) < 1e-12
    report = [ln for ln in full.stdout.splitlines() if ln.startswith("coherence:")]
    assert len(report) == 1 and "mean rate" in report[0]
    # a file with accumulators without --coherence: refused, the message names the flag, nothing is saved
    down = run("--resume", "part.pt", "--save", "never.pt", "--log", "bad.csv")
    assert down.returncode != 0 and "--coherence" in down.stderr and "accumulators" in down.stderr
    assert not os.path.exists(tmp_path / "never.pt")
    # a plain file with --coherence: continues with fresh accumulators and says so
    plain3 = run("--stop-epoch", "3", "--save", "plain3.pt", "--log", "p3.csv")
    assert plain3.returncode == 0, plain3.stderr[-2000:]
    assert not any(ln.startswith("coherence:") for ln in plain3.stdout.splitlines())
    c, p = load(tmp_path, "plain3.pt"), load(tmp_path, "part.pt")
    assert "coherence" not in c and c["kind"] == p["kind"] == "ntuple6_afterstate" and c["train"] == p["train"]
    assert not same(p["weights"], c["weights"]), "the same command without the flag trains the same values"
    del c, p
    up = run("--coherence", "--resume", "plain3.pt", "--save", "up.pt", "--log", "up.csv")
    assert up.returncode == 0, up.stderr[-2000:]
    assert "start at zero" in up.stdout
    u, p3 = load(tmp_path, "up.pt"), load(tmp_path, "plain3.pt")
    assert u["train"]["epoch"] == 6 and tuple(u["coherence"].shape) == ACC_SHAPE and bool(u["coherence"].any())
    assert not same(u["weights"], p3["weights"]) and u["ctr"] > p3["ctr"]
    del u, p3
    os.remove(tmp_path / "up.pt")
    # --coherence with any other agent, and in the one-env loop: refused with a message that says so
    for agent in ("hash", "row-tuple", "line-tuple", "afterstate"):
        bad = script(tmp_path, "cpu", "train.py", "--agent", agent, "--num-envs", "64", "--episodes", "2", "--coherence",
                     "--save", "never.pt", "--log", "bad.csv")
        assert bad.returncode != 0 and "--coherence applies to --agent ntuple" in bad.stderr and agent in bad.stderr, agent
    bad = script(tmp_path, "cpu", "train.py", "--agent", "ntuple", "--num-envs", "1", "--episodes", "2", "--coherence")
    assert bad.returncode != 0 and "--coherence" in bad.stderr
    assert not os.path.exists(tmp_path / "never.pt")
    # evaluate.py dispatches on the kind: a TC file plays as a plain one, with --fused and with --fused --search
    common = ("evaluate.py", "--model", "full.pt", "--num-envs", "96", "--episodes", "1", "--steps-per-launch", "32")
    x, y, z = (script(tmp_path, "cpu", *common, *f) for f in ((), ("--fused",), ("--fused", "--search")))
    for r in (x, y, z):
        assert r.returncode == 0, r.stderr[-2000:]
    x, y, z = (last_json(r) for r in (x, y, z))
    assert x["agent"] == y["agent"] == z["agent"] == "ntuple" and y["fused"] is True and z["fused"] is True
    for key in S.KEYS:
        assert x[key] == y[key], key
    assert z["games"] >= 96 and x["games"] >= 96
    # ... and the games are those of the same values in a file without accumulators
    torch.save({k: v for k, v in a.items() if k != "coherence"}, tmp_path / "stripped.pt")
    del a
    w = script(tmp_path, "cpu", "evaluate.py", "--model", "stripped.pt", "--num-envs", "96", "--episodes", "1",
               "--steps-per-launch", "32", "--fused")
    assert w.returncode == 0, w.stderr[-2000:]
    for key in S.KEYS:
        assert last_json(w)[key] == y[key], key


@pytest.mark.gpu
def test_the_scripts_on_the_device(pkg, tmp_path):
    t = script(tmp_path, "cuda", "train.py", "--agent", "ntuple", "--coherence", "--alpha", "0.5", "--num-envs", "1024",
               "--episodes", "3", "--report-every", "1", "--save", "g.pt", "--log", "g.csv", "--eval-every", "1",
               "--eval-envs", "512", "--eval-log", "E.jsonl")
    assert t.returncode == 0, t.stderr[-2000:]
    lines = [json.loads(ln) for ln in open(tmp_path / "E.jsonl").read().splitlines()]
    assert [ln["epoch"] for ln in lines] == [1, 2, 3] and all(0.0 < ln["coherence_mean_rate"] <= 1.0 for ln in lines)
    g = load(tmp_path, "g.pt")
    E, A = g["coherence"][..., 0], g["coherence"][..., 1]
    assert bool((A > 0).any()) and bool((E.abs() <= A).all()) and bool(torch.isfinite(g["coherence"]).all())
    del g, E, A
    y = script(tmp_path, "cuda", "evaluate.py", "--model", "g.pt", "--num-envs", "1024", "--episodes", "1", "--fused", "--search")
    assert y.returncode == 0, y.stderr[-2000:]
    assert last_json(y)["agent"] == "ntuple" and last_json(y)["games"] >= 1024
    down = script(tmp_path, "cuda", "train.py", "--agent", "ntuple", "--num-envs", "1024", "--episodes", "6", "--resume", "g.pt")
    assert down.returncode != 0 and "--coherence" in down.stderr
