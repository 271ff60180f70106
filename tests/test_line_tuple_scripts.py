"""The line-tuple learner through the scripts: `train.py --agent line-tuple --save / --resume / --eval-every`, the
promotion of a row-tuple file by `--resume`, `evaluate.py --model` on a line-tuple file with and without `--fused`, and
merge_tables.py's refusal of one.  As subprocesses on the CPU twin with one host thread (a learning run is then
sequential and reproducible), and once on the GPU.  The helpers are those of the row-tuple learner's script test."""
import json
import os

import pytest
import torch

import test_row_tuple_player as P

script, load, log_rows, bits = P.script, P.load, P.log_rows, P.bits
KEYS = ("games", "env_steps", "mean_score", "max_tile_hist", "valid_move_frac")


def last_json(run):
    return json.loads(run.stdout.strip().splitlines()[-1])


def test_train_save_resume_eval_and_the_other_scripts(pkg, tmp_path):
    train = ("train.py", "--agent", "line-tuple", "--num-envs", "64", "--episodes", "6", "--seed", "4", "--report-every", "1")
    run = lambda *a: script(tmp_path, "cpu", *train, *a)   # noqa: E731
    full = run("--save", "full.pt", "--log", "full.csv")
    assert full.returncode == 0, full.stderr[-2000:]
    part = run("--stop-epoch", "3", "--save", "part.pt", "--log", "p1.csv")
    assert part.returncode == 0, part.stderr[-2000:]
    rest = run("--resume", "part.pt", "--save", "resumed.pt", "--log", "p2.csv")
    assert rest.returncode == 0, rest.stderr[-2000:]
    a, b, p = (load(tmp_path, f) for f in ("full.pt", "resumed.pt", "part.pt"))
    assert a["kind"] == "line_tuple" and tuple(a["weights"].shape) == (8, 65536, 4)
    assert 3 <= p["train"]["epoch"] < 6 == a["train"]["epoch"] == b["train"]["epoch"]
    assert torch.equal(bits(a["weights"]), bits(b["weights"])) and bool(a["weights"][:4].any()) and bool(a["weights"][4:].any())
    assert not torch.equal(bits(a["weights"]), bits(p["weights"]))
    assert a["ctr"] == b["ctr"] and torch.equal(a["stats_i"], b["stats_i"]) and torch.equal(a["stats_f"], b["stats_f"])
    assert a["schedule"] == b["schedule"]
    assert torch.equal(a["env"]["boards"], b["env"]["boards"]) and torch.equal(a["env"]["aux"], b["env"]["aux"])
    rows = log_rows(tmp_path, "full.csv")
    assert log_rows(tmp_path, "p1.csv") + log_rows(tmp_path, "p2.csv") == rows and rows[-1][0] == "6"
    # --eval-every: one JSON line per evaluation, the training log and the saved weights as without it
    ev = run("--save", "ev.pt", "--log", "ev.csv", "--eval-every", "2", "--eval-envs", "128", "--eval-log", "E.jsonl")
    assert ev.returncode == 0, ev.stderr[-2000:]
    e = load(tmp_path, "ev.pt")
    assert torch.equal(bits(a["weights"]), bits(e["weights"])) and log_rows(tmp_path, "ev.csv") == rows
    assert a["ctr"] == e["ctr"] and torch.equal(a["stats_i"], e["stats_i"]) and torch.equal(a["env"]["aux"], e["env"]["aux"])
    lines = [json.loads(ln) for ln in open(tmp_path / "E.jsonl").read().splitlines()]
    assert [ln["epoch"] for ln in lines] == [2, 4, 6]
    for ln in lines:
        assert ln["games"] >= 128 and sum(ln["max_tile_hist"].values()) == ln["games"] and 0.0 < ln["valid_move_frac"] <= 1.0
    # the switches the row-tuple learner refuses are refused here too
    for flag in (("--deterministic",), ("--episode-log", "ep.csv"), ("--symmetric",), ("--unfold", "--resume", "full.pt")):
        bad = run(*flag, "--log", "bad.csv")
        assert bad.returncode != 0 and flag[0] in bad.stderr, flag
    # evaluate.py reads the kind from the file: the same games with --fused and without, and the reference policy
    common = ("evaluate.py", "--model", "full.pt", "--num-envs", "96", "--episodes", "1", "--steps-per-launch", "32")
    plain, fused, ref = (script(tmp_path, "cpu", *common, *x) for x in ((), ("--fused",), ("--policy", "reference")))
    for r in (plain, fused, ref):
        assert r.returncode == 0, r.stderr[-2000:]
    x, y, z = (last_json(r) for r in (plain, fused, ref))
    assert x["agent"] == y["agent"] == z["agent"] == "line-tuple" and y["fused"] is True and "rows" not in x
    assert set(y) == set(x) | {"fused"}
    for key in KEYS:
        assert x[key] == y[key], key
    assert x["games"] >= 96 and x["valid_move_frac"] > z["valid_move_frac"]
    # PROMOTION: --resume of a row-tuple file under --agent line-tuple; the rows go on learning with columns
    rt = script(tmp_path, "cpu", "train.py", "--agent", "row-tuple", "--num-envs", "64", "--episodes", "6", "--seed", "4",
                "--report-every", "1", "--stop-epoch", "3", "--save", "rt.pt", "--log", "rt.csv")
    assert rt.returncode == 0, rt.stderr[-2000:]
    pro = run("--resume", "rt.pt", "--save", "pro.pt", "--log", "pro.csv")
    assert pro.returncode == 0 and "promoted" in pro.stdout, pro.stderr[-2000:]
    r, q = load(tmp_path, "rt.pt"), load(tmp_path, "pro.pt")
    assert r["kind"] == "row_tuple" and q["kind"] == "line_tuple" and q["train"]["epoch"] == 6 > r["train"]["epoch"] >= 3
    assert q["ctr"] > r["ctr"] and int(q["stats_i"][1]) > int(r["stats_i"][1]) and bool(q["weights"][4:].any())
    assert last_json(script(tmp_path, "cpu", "evaluate.py", "--model", "rt.pt", "--num-envs", "64"))["agent"] == "row-tuple"
    # the other directions are refused: a line-tuple file under --agent row-tuple or hash, a hash file here, a merge
    h = script(tmp_path, "cpu", "train.py", "--num-envs", "64", "--steps-per-launch", "32", "--episodes", "2", "--max-steps",
               "64", "--capacity-log2", "14", "--save", "h.pt", "--log", "h.csv")
    assert h.returncode == 0, h.stderr[-2000:]
    assert run("--resume", "h.pt", "--log", "bad.csv").returncode != 0
    for agent in ("row-tuple", "hash"):
        down = script(tmp_path, "cpu", "train.py", "--agent", agent, "--num-envs", "64", "--episodes", "6", "--resume",
                      "full.pt", "--log", "bad.csv")
        assert down.returncode != 0 and "do not load into each other" in down.stderr, agent
    merge = script(tmp_path, "cpu", "merge_tables.py", "full.pt", "resumed.pt", "--out", "m.pt")
    assert merge.returncode != 0 and "line-tuple weights" in merge.stderr and "not built" in merge.stderr
    assert not os.path.exists(tmp_path / "m.pt")


@pytest.mark.gpu
def test_the_scripts_on_the_device(pkg, tmp_path):
    t = script(tmp_path, "cuda", "train.py", "--agent", "line-tuple", "--num-envs", "1024", "--episodes", "3", "--report-every",
               "1", "--save", "g.pt", "--log", "g.csv", "--eval-every", "1", "--eval-envs", "512", "--eval-log", "E.jsonl")
    assert t.returncode == 0, t.stderr[-2000:]
    assert [json.loads(ln)["epoch"] for ln in open(tmp_path / "E.jsonl").read().splitlines()] == [1, 2, 3]
    g = load(tmp_path, "g.pt")
    assert g["kind"] == "line_tuple" and bool(g["weights"][:4].any()) and bool(g["weights"][4:].any())
    common = ("evaluate.py", "--model", "g.pt", "--num-envs", "1024", "--episodes", "1")
    plain, fused = script(tmp_path, "cuda", *common), script(tmp_path, "cuda", *common, "--fused")
    assert plain.returncode == 0 and fused.returncode == 0, plain.stderr[-2000:] + fused.stderr[-2000:]
    x, y = (last_json(r) for r in (plain, fused))
    assert y["agent"] == "line-tuple" and y["fused"] is True and y["games"] >= 1024
    for key in KEYS:
        assert x[key] == y[key], key
    more = script(tmp_path, "cuda", "train.py", "--agent", "line-tuple", "--num-envs", "1024", "--episodes", "6", "--resume",
                  "g.pt", "--report-every", "1", "--save", "g2.pt", "--log", "g2.csv")
    assert more.returncode == 0, more.stderr[-2000:]
    g2 = load(tmp_path, "g2.pt")
    assert 3 <= g["train"]["epoch"] < 6 == g2["train"]["epoch"] and g2["ctr"] > g["ctr"]
    merge = script(tmp_path, "cuda", "merge_tables.py", "g.pt", "g2.pt", "--out", "m.pt")
    assert merge.returncode != 0 and "line-tuple weights" in merge.stderr
