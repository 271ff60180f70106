"""The 6-tuple afterstate network through the scripts: `train.py --agent ntuple --save / --resume / --eval-every`,
`evaluate.py --model` on its file with and without `--fused`, the refusals of every crossing of kinds, and
merge_tables.py's refusal.  As subprocesses on the CPU twin with one host thread (a learning run is then sequential and
reproducible), and once on the GPU.  The helpers are those of the row-tuple learner's script test.  Small runs: every
file written is 256 MiB, so each run's file replaces the one before where the test no longer needs it."""
import json
import os

import pytest
import torch

import test_row_tuple_player as P

script, load, log_rows, bits = P.script, P.load, P.log_rows, P.bits
KEYS = ("games", "env_steps", "mean_score", "max_tile_hist", "valid_move_frac")
SHAPE = (4, 1 << 24)


def last_json(run):
    return json.loads(run.stdout.strip().splitlines()[-1])


def same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_train_save_resume_eval_and_the_other_scripts(pkg, tmp_path):
    train = ("train.py", "--agent", "ntuple", "--num-envs", "64", "--episodes", "6", "--seed", "4", "--report-every", "1")
    run = lambda *a: script(tmp_path, "cpu", *train, *a)   # noqa: E731
    full = run("--save", "full.pt", "--log", "full.csv")
    assert full.returncode == 0, full.stderr[-2000:]
    part = run("--stop-epoch", "3", "--save", "part.pt", "--log", "p1.csv")
    assert part.returncode == 0, part.stderr[-2000:]
    rest = run("--resume", "part.pt", "--save", "resumed.pt", "--log", "p2.csv")
    assert rest.returncode == 0, rest.stderr[-2000:]
    a, p = load(tmp_path, "full.pt"), load(tmp_path, "part.pt")
    assert a["kind"] == "ntuple6_afterstate" and tuple(a["weights"].shape) == SHAPE and a["weights"].dtype == torch.float32
    assert not same(a["weights"], p["weights"]) and 3 <= p["train"]["epoch"] < 6 == a["train"]["epoch"]
    del p
    b = load(tmp_path, "resumed.pt")
    assert b["train"]["epoch"] == 6
    assert same(a["weights"], b["weights"]) and all(bool(a["weights"][k].any()) for k in range(4))
    assert a["ctr"] == b["ctr"] and torch.equal(a["stats_i"], b["stats_i"]) and torch.equal(a["stats_f"], b["stats_f"])
    assert a["schedule"] == b["schedule"]
    assert torch.equal(a["env"]["boards"], b["env"]["boards"]) and torch.equal(a["env"]["aux"], b["env"]["aux"])
    del b
    rows = log_rows(tmp_path, "full.csv")
    assert log_rows(tmp_path, "p1.csv") + log_rows(tmp_path, "p2.csv") == rows and rows[-1][0] == "6"
    # --eval-every: one JSON line per evaluation, the training log and the saved values as without it
    ev = run("--save", "resumed.pt", "--log", "ev.csv", "--eval-every", "3", "--eval-envs", "128", "--eval-log", "E.jsonl")
    assert ev.returncode == 0, ev.stderr[-2000:]
    e = load(tmp_path, "resumed.pt")
    assert same(a["weights"], e["weights"]) and log_rows(tmp_path, "ev.csv") == rows
    assert a["ctr"] == e["ctr"] and torch.equal(a["stats_i"], e["stats_i"]) and torch.equal(a["env"]["aux"], e["env"]["aux"])
    del a, e
    lines = [json.loads(ln) for ln in open(tmp_path / "E.jsonl").read().splitlines()]
    assert [ln["epoch"] for ln in lines] == [3, 6]
    for ln in lines:
        assert ln["games"] >= 128 and sum(ln["max_tile_hist"].values()) == ln["games"] and 0.0 < ln["valid_move_frac"] <= 1.0
    # the switches the other weights learners refuse are refused here too
    for flag in (("--deterministic",), ("--episode-log", "ep.csv"), ("--symmetric",), ("--fold", "mean", "--resume", "full.pt"),
                 ("--unfold", "--resume", "full.pt")):
        bad = run(*flag, "--log", "bad.csv")
        assert bad.returncode != 0 and flag[0] in bad.stderr, flag
    # evaluate.py reads the kind from the file: the same games with --fused and without
    common = ("evaluate.py", "--model", "full.pt", "--num-envs", "96", "--episodes", "1", "--steps-per-launch", "32")
    plain, fused = (script(tmp_path, "cpu", *common, *x) for x in ((), ("--fused",)))
    for r in (plain, fused):
        assert r.returncode == 0, r.stderr[-2000:]
    x, y = (last_json(r) for r in (plain, fused))
    assert x["agent"] == y["agent"] == "ntuple" and y["fused"] is True and "rows" not in x
    assert set(y) == set(x) | {"fused"}
    for key in KEYS:
        assert x[key] == y[key], key
    assert x["games"] >= 96
    # every crossing of kinds is refused, in both directions, and so is a merge
    others = {"row-tuple": "rowtuple.pt", "line-tuple": "linetuple.pt", "afterstate": "afterstate.pt", "hash": "h.pt"}
    torch.save(pkg.BatchedRowTupleAgent(6, device="cpu").state_dict(), tmp_path / "rowtuple.pt")
    torch.save(pkg.BatchedLineTupleAgent(6, device="cpu").state_dict(), tmp_path / "linetuple.pt")
    torch.save(pkg.BatchedAfterstateAgent(6, device="cpu").state_dict(), tmp_path / "afterstate.pt")
    torch.save(pkg.BatchedQLearningAgent(6, capacity_log2=12, device="cpu", placement="plain").state_dict(), tmp_path / "h.pt")
    for agent, name in others.items():
        up = run("--resume", name, "--save", "never.pt", "--log", "bad.csv")
        assert up.returncode != 0 and "do not load into each other" in up.stderr, f"{agent} file into the 6-tuple network"
        down = script(tmp_path, "cpu", "train.py", "--agent", agent, "--num-envs", "64", "--episodes", "6", "--resume",
                      "full.pt", "--save", "never.pt", "--log", "bad.csv")
        assert down.returncode != 0 and "do not load into each other" in down.stderr, f"6-tuple file into {agent}"
    assert not os.path.exists(tmp_path / "never.pt")
    merge = script(tmp_path, "cpu", "merge_tables.py", "full.pt", "resumed.pt", "--out", "m.pt")
    assert merge.returncode != 0 and "6-tuple afterstate network" in merge.stderr and "not built" in merge.stderr
    assert not os.path.exists(tmp_path / "m.pt")


@pytest.mark.gpu
def test_the_scripts_on_the_device(pkg, tmp_path):
    t = script(tmp_path, "cuda", "train.py", "--agent", "ntuple", "--num-envs", "1024", "--episodes", "3", "--report-every",
               "1", "--save", "g.pt", "--log", "g.csv", "--eval-every", "1", "--eval-envs", "512", "--eval-log", "E.jsonl")
    assert t.returncode == 0, t.stderr[-2000:]
    assert [json.loads(ln)["epoch"] for ln in open(tmp_path / "E.jsonl").read().splitlines()] == [1, 2, 3]
    common = ("evaluate.py", "--model", "g.pt", "--num-envs", "1024", "--episodes", "1")
    plain, fused = script(tmp_path, "cuda", *common), script(tmp_path, "cuda", *common, "--fused")
    assert plain.returncode == 0 and fused.returncode == 0, plain.stderr[-2000:] + fused.stderr[-2000:]
    x, y = (last_json(r) for r in (plain, fused))
    assert y["agent"] == "ntuple" and y["fused"] is True and y["games"] >= 1024
    for key in KEYS:
        assert x[key] == y[key], key
    more = script(tmp_path, "cuda", "train.py", "--agent", "ntuple", "--num-envs", "1024", "--episodes", "6", "--resume",
                  "g.pt", "--report-every", "1", "--save", "g2.pt", "--log", "g2.csv")
    assert more.returncode == 0, more.stderr[-2000:]
    g = load(tmp_path, "g.pt")
    assert g["kind"] == "ntuple6_afterstate" and all(bool(g["weights"][k].any()) for k in range(4))
    epoch, ctr = g["train"]["epoch"], g["ctr"]
    del g
    g2 = load(tmp_path, "g2.pt")
    assert 3 <= epoch < 6 == g2["train"]["epoch"] and g2["ctr"] > ctr
    del g2
    merge = script(tmp_path, "cuda", "merge_tables.py", "g.pt", "g2.pt", "--out", "m.pt")
    assert merge.returncode != 0 and "6-tuple afterstate network" in merge.stderr
