"""TD(lambda) through the scripts: `train.py --agent ntuple --trace-lambda L [--trace-depth H] --save / --resume` (two
halves of a run give the log rows, the weights and the traces of the whole run), the refusals of the flags, and
`evaluate.py --model` on the saved file with and without `--fused --search`.  As subprocesses on the CPU twin with one
host thread (a learning run is then sequential and reproducible)."""
import os

import pytest
import torch

import test_ntuple_scripts as S
import test_row_tuple_player as P

script, load, log_rows, same, last_json = P.script, P.load, P.log_rows, S.same, S.last_json


def test_train_save_resume_and_evaluate(pkg, tmp_path):
    train = ("train.py", "--agent", "ntuple", "--num-envs", "64", "--episodes", "6", "--seed", "4", "--report-every", "1",
             "--alpha", "0.5")
    run = lambda *a: script(tmp_path, "cpu", *train, *a)   # noqa: E731
    full = run("--trace-lambda", "0.5", "--save", "full.pt", "--log", "full.csv")
    assert full.returncode == 0, full.stderr[-2000:]
    part = run("--trace-lambda", "0.5", "--stop-epoch", "3", "--save", "part.pt", "--log", "p1.csv")
    assert part.returncode == 0, part.stderr[-2000:]
    rest = run("--trace-lambda", "0.5", "--resume", "part.pt", "--save", "resumed.pt", "--log", "p2.csv")
    assert rest.returncode == 0, rest.stderr[-2000:]
    a, p = load(tmp_path, "full.pt"), load(tmp_path, "part.pt")
    assert a["kind"] == "ntuple6_afterstate" and a["train"]["epoch"] == 6
    for sd in (a, p):
        tr = sd["trace"]
        assert tr["lambda"] == 0.5 and tr["depth"] == 3 and tr["keys"].dtype == torch.int64 and tuple(tr["keys"].shape) == (64, 4)
        n = tr["keys"][:, 0]
        assert bool(((n >= 0) & (n <= 3)).all()) and bool((tr["keys"][:, 1:][torch.arange(1, 4)[None, :] > n[:, None]] == 0).all())
    assert bool((p["trace"]["keys"][:, 0] > 0).any()), "no trace is in flight at the checkpoint"
    # save at epoch 3 + resume == the uninterrupted run: values, traces, counters, statistics, boards, the log
    b = load(tmp_path, "resumed.pt")
    assert b["train"]["epoch"] == 6 and same(a["weights"], b["weights"]) and torch.equal(a["trace"]["keys"], b["trace"]["keys"])
    assert a["ctr"] == b["ctr"] and torch.equal(a["stats_i"], b["stats_i"]) and torch.equal(a["stats_f"], b["stats_f"])
    assert torch.equal(a["env"]["boards"], b["env"]["boards"]) and torch.equal(a["env"]["aux"], b["env"]["aux"])
    del b
    os.remove(tmp_path / "resumed.pt")
    assert log_rows(tmp_path, "p1.csv") + log_rows(tmp_path, "p2.csv") == log_rows(tmp_path, "full.csv")
    # the same command without the flag trains other values; --trace-depth 0 trains the plain learner's
    plain = run("--stop-epoch", "3", "--save", "plain3.pt", "--log", "p3.csv")
    flat = run("--trace-lambda", "0.5", "--trace-depth", "0", "--stop-epoch", "3", "--save", "flat3.pt", "--log", "p4.csv")
    assert plain.returncode == 0 and flat.returncode == 0, plain.stderr[-2000:] + flat.stderr[-2000:]
    c, f = load(tmp_path, "plain3.pt"), load(tmp_path, "flat3.pt")
    assert "trace" not in c and c["train"] == p["train"] and not same(p["weights"], c["weights"])
    assert same(f["weights"], c["weights"]) and f["trace"]["depth"] == 0 and log_rows(tmp_path, "p3.csv") == log_rows(tmp_path, "p4.csv")
    del c, f, p
    # a file with traces without --trace-lambda: refused, the message names the flag, nothing is saved; a plain file
    # with the flag continues with empty traces; another depth is refused
    down = run("--resume", "part.pt", "--save", "never.pt", "--log", "bad.csv")
    assert down.returncode != 0 and "--trace-lambda" in down.stderr and "traces" in down.stderr
    up = run("--trace-lambda", "0.5", "--resume", "plain3.pt", "--save", "up.pt", "--log", "up.csv")
    assert up.returncode == 0, up.stderr[-2000:]
    assert load(tmp_path, "up.pt")["train"]["epoch"] == 6
    os.remove(tmp_path / "up.pt")
    other = run("--trace-lambda", "0.5", "--trace-depth", "2", "--resume", "part.pt", "--save", "never.pt", "--log", "bad.csv")
    assert other.returncode != 0 and "depth" in other.stderr
    assert not os.path.exists(tmp_path / "never.pt")
    # evaluate.py dispatches on the kind: a file with traces plays as a plain one, with --fused and with --fused --search
    common = ("evaluate.py", "--model", "full.pt", "--num-envs", "96", "--episodes", "1", "--steps-per-launch", "32")
    x, y, z = (script(tmp_path, "cpu", *common, *fl) for fl in ((), ("--fused",), ("--fused", "--search")))
    for r in (x, y, z):
        assert r.returncode == 0, r.stderr[-2000:]
    x, y, z = (last_json(r) for r in (x, y, z))
    assert x["agent"] == y["agent"] == z["agent"] == "ntuple" and y["fused"] is True and z["fused"] is True
    for key in S.KEYS:
        assert x[key] == y[key], key
    assert z["games"] >= 96 and x["games"] >= 96
    torch.save({k: v for k, v in a.items() if k != "trace"}, tmp_path / "stripped.pt")
    w = script(tmp_path, "cpu", "evaluate.py", "--model", "stripped.pt", "--num-envs", "96", "--episodes", "1",
               "--steps-per-launch", "32", "--fused")
    assert w.returncode == 0, w.stderr[-2000:]
    for key in S.KEYS:
        assert last_json(w)[key] == y[key], key


def test_command_line_refusals(pkg, tmp_path):
    """--trace-lambda with --coherence, with --stage-tiles, with every other agent, in the one-env loop, out of range; and
    --trace-depth without it or out of range: refused with a message that says so, nothing saved."""
    base = ("train.py", "--num-envs", "64", "--episodes", "2", "--save", "never.pt", "--log", "bad.csv")
    for agent in ("hash", "row-tuple", "line-tuple", "afterstate"):
        bad = script(tmp_path, "cpu", *base, "--agent", agent, "--trace-lambda", "0.5")
        assert bad.returncode != 0 and "--trace-lambda applies to --agent ntuple" in bad.stderr and agent in bad.stderr, agent
    nt = base + ("--agent", "ntuple")
    for extra, word in ((("--trace-lambda", "0.5", "--coherence"), "--coherence"),
                        (("--trace-lambda", "0.5", "--stage-tiles", "2048"), "--stage-tiles"),
                        (("--trace-lambda", "1.5"), "[0, 1]"), (("--trace-lambda", "-0.1"), "[0, 1]"),
                        (("--trace-lambda", "nan"), "[0, 1]"), (("--trace-lambda", "0.5", "--trace-depth", "4"), "--trace-depth"),
                        (("--trace-lambda", "0.5", "--trace-depth", "-1"), "--trace-depth"),
                        (("--trace-depth", "2"), "--trace-lambda")):
        bad = script(tmp_path, "cpu", *nt, *extra)
        assert bad.returncode != 0 and word in bad.stderr, extra
    bad = script(tmp_path, "cpu", "train.py", "--agent", "ntuple", "--num-envs", "1", "--episodes", "2", "--trace-lambda", "0.5")
    assert bad.returncode != 0 and "--trace-lambda" in bad.stderr
    assert not os.path.exists(tmp_path / "never.pt")


@pytest.mark.gpu
def test_the_scripts_on_the_device(pkg, tmp_path):
    t = script(tmp_path, "cuda", "train.py", "--agent", "ntuple", "--trace-lambda", "0.5", "--alpha", "0.5", "--num-envs",
               "1024", "--episodes", "3", "--report-every", "1", "--save", "g.pt", "--log", "g.csv")
    assert t.returncode == 0, t.stderr[-2000:]
    g = load(tmp_path, "g.pt")
    keys = g["trace"]["keys"]
    n = keys[:, 0]
    assert tuple(keys.shape) == (1024, 4) and bool(((n >= 0) & (n <= 3)).all()) and bool((n > 0).any())
    assert bool((keys[:, 1:][torch.arange(1, 4)[None, :] > n[:, None]] == 0).all()) and bool(torch.isfinite(g["weights"]).all())
    del g
    y = script(tmp_path, "cuda", "evaluate.py", "--model", "g.pt", "--num-envs", "1024", "--episodes", "1", "--fused", "--search")
    assert y.returncode == 0, y.stderr[-2000:]
    assert last_json(y)["agent"] == "ntuple" and last_json(y)["games"] >= 1024
    down = script(tmp_path, "cuda", "train.py", "--agent", "ntuple", "--num-envs", "1024", "--episodes", "6", "--resume", "g.pt")
    assert down.returncode != 0 and "--trace-lambda" in down.stderr
