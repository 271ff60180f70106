"""The synchronous batch step through the scripts: `train.py --agent ntuple --synchronous` saved with one and with four
host threads (the same bytes), `--save` / `--resume` (two halves of a run give the log rows and the weights of the whole
run), the refusals of the flag, and `evaluate.py --fused` on the saved file.  As subprocesses on the CPU twin.  (At 512
envs the twin's work rule gives one range whatever Q2048_HOST_THREADS says; ranges that really differ are
test_ntuple_sync.py::test_cpu_twin_does_not_depend_on_its_threads.)"""
import os
import subprocess
import sys

import pytest
import torch

import test_ntuple_scripts as S
import test_row_tuple_player as P

REPO, load, log_rows, same, last_json = P.REPO, P.load, P.log_rows, S.same, S.last_json


def script(tmp_path, device, threads, name, *a):
    env = dict(os.environ, Q2048_HOST_THREADS=str(threads))
    return subprocess.run([sys.executable, os.path.join(REPO, name), "--device", device, *a], capture_output=True,
                          text=True, timeout=600, cwd=str(tmp_path), env=env)


def test_train_threads_save_resume_and_evaluate(pkg, tmp_path):
    train = ("train.py", "--agent", "ntuple", "--synchronous", "--num-envs", "512", "--episodes", "6", "--seed", "4",
             "--report-every", "1")
    run = lambda threads, *a: script(tmp_path, "cpu", threads, *train, *a)   # noqa: E731
    full = run(1, "--save", "full.pt", "--log", "full.csv")
    assert full.returncode == 0, full.stderr[-2000:]
    four = run(4, "--save", "four.pt", "--log", "four.csv")
    assert four.returncode == 0, four.stderr[-2000:]
    a, b = load(tmp_path, "full.pt"), load(tmp_path, "four.pt")
    assert a["kind"] == "ntuple6_afterstate" and a["train"]["epoch"] == 6 and bool(a["weights"].any())
    assert not any("sync" in k or k in ("acc", "pend") for k in a), "the accumulators are never saved"
    assert same(a["weights"], b["weights"]) and a["ctr"] == b["ctr"] and torch.equal(a["stats_i"], b["stats_i"])
    assert torch.equal(a["env"]["boards"], b["env"]["boards"]) and torch.equal(a["env"]["aux"], b["env"]["aux"])
    assert log_rows(tmp_path, "full.csv") == log_rows(tmp_path, "four.csv")
    del b
    os.remove(tmp_path / "four.pt")
    # save at epoch 3 + resume == the uninterrupted run (the second half with four threads)
    part = run(1, "--stop-epoch", "3", "--save", "part.pt", "--log", "p1.csv")
    assert part.returncode == 0, part.stderr[-2000:]
    rest = run(4, "--resume", "part.pt", "--save", "resumed.pt", "--log", "p2.csv")
    assert rest.returncode == 0, rest.stderr[-2000:]
    b = load(tmp_path, "resumed.pt")
    assert b["train"]["epoch"] == 6 and same(a["weights"], b["weights"])
    assert a["ctr"] == b["ctr"] and torch.equal(a["stats_i"], b["stats_i"]) and torch.equal(a["stats_f"], b["stats_f"])
    assert torch.equal(a["env"]["boards"], b["env"]["boards"]) and torch.equal(a["env"]["aux"], b["env"]["aux"])
    assert log_rows(tmp_path, "p1.csv") + log_rows(tmp_path, "p2.csv") == log_rows(tmp_path, "full.csv")
    del b
    os.remove(tmp_path / "resumed.pt")
    # the same command without the flag trains other values, and continues the synchronous learner's file (and back)
    plain = script(tmp_path, "cpu", 1, *(x for x in train if x != "--synchronous"), "--stop-epoch", "3", "--save",
                   "plain3.pt", "--log", "p3.csv")
    assert plain.returncode == 0, plain.stderr[-2000:]
    p, c = load(tmp_path, "part.pt"), load(tmp_path, "plain3.pt")
    assert set(p) == set(c) and not same(p["weights"], c["weights"])
    del p, c
    up = run(1, "--resume", "plain3.pt", "--save", "up.pt", "--log", "up.csv")
    assert up.returncode == 0, up.stderr[-2000:]
    assert load(tmp_path, "up.pt")["train"]["epoch"] == 6
    os.remove(tmp_path / "up.pt")
    # evaluate.py plays the file: with --fused the same games as without
    common = ("evaluate.py", "--model", "full.pt", "--num-envs", "96", "--episodes", "1", "--steps-per-launch", "32")
    x, y = (script(tmp_path, "cpu", 1, *common, *fl) for fl in ((), ("--fused",)))
    for r in (x, y):
        assert r.returncode == 0, r.stderr[-2000:]
    x, y = last_json(x), last_json(y)
    assert x["agent"] == y["agent"] == "ntuple" and y["fused"] is True and y["games"] >= 96
    for key in S.KEYS:
        assert x[key] == y[key], key


def test_command_line_refusals(pkg, tmp_path):
    """--synchronous with every other agent, with --coherence, --stage-tiles, --carousel and --trace-lambda, and in the
    one-env loop: refused with a message that names the flag, nothing saved.  --deterministic stays the hash-table
    agent's."""
    base = ("train.py", "--num-envs", "64", "--episodes", "2", "--save", "never.pt", "--log", "bad.csv")
    for agent in ("hash", "row-tuple", "line-tuple", "afterstate"):
        bad = script(tmp_path, "cpu", 1, *base, "--agent", agent, "--synchronous")
        assert bad.returncode != 0 and "--synchronous applies to --agent ntuple" in bad.stderr and agent in bad.stderr, agent
    nt = base + ("--agent", "ntuple", "--synchronous")
    for extra, word in ((("--coherence",), "--coherence"), (("--stage-tiles", "2048"), "--stage-tiles"),
                        (("--stage-tiles", "2048", "--carousel", "8"), "--stage-tiles"), (("--carousel", "8"), "--carousel"),
                        (("--trace-lambda", "0.5"), "--trace-lambda"), (("--deterministic",), "--deterministic")):
        bad = script(tmp_path, "cpu", 1, *nt, *extra)
        assert bad.returncode != 0 and word in bad.stderr, extra
        assert "--synchronous" in bad.stderr or extra == ("--deterministic",), extra
    bad = script(tmp_path, "cpu", 1, "train.py", "--agent", "ntuple", "--num-envs", "1", "--episodes", "2", "--synchronous")
    assert bad.returncode != 0 and "--synchronous" in bad.stderr
    assert not os.path.exists(tmp_path / "never.pt")


@pytest.mark.gpu
def test_the_scripts_on_the_device(pkg, tmp_path):
    """Two runs of the same command on the device save the same bytes, and they are the CPU twin's.  (evaluate.py on such
    a file: the CPU test above; the file is a plain network's.)"""
    train = ("train.py", "--agent", "ntuple", "--synchronous", "--num-envs", "512", "--episodes", "2", "--report-every", "1")
    for dev, name in (("cuda", "g1"), ("cuda", "g2"), ("cpu", "c")):
        t = script(tmp_path, dev, 4, *train, "--save", name + ".pt", "--log", name + ".csv")
        assert t.returncode == 0, t.stderr[-2000:]
    g1, g2, c = (load(tmp_path, n + ".pt") for n in ("g1", "g2", "c"))
    assert bool(g1["weights"].any()) and bool(torch.isfinite(g1["weights"]).all())
    for other in (g2, c):
        assert same(g1["weights"], other["weights"]) and torch.equal(g1["env"]["boards"], other["env"]["boards"])
        assert torch.equal(g1["stats_i"], other["stats_i"])
    del g1, g2, c
