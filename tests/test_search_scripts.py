"""`evaluate.py --search`: the one-level expectimax player through the script, on a tiny file saved by `train.py --agent
afterstate`, and its refusals -- without `--fused`, on a hash-table file, on a row-tuple file.  As subprocesses on the CPU
twin, and once on the GPU.  The helpers are those of the row-tuple learner's script test."""
import json

import pytest
import torch

import test_row_tuple_player as P

script = P.script


def last_json(run):
    return json.loads(run.stdout.strip().splitlines()[-1])


def train_afterstate(tmp_path, device, envs):
    t = script(tmp_path, device, "train.py", "--agent", "afterstate", "--num-envs", str(envs), "--episodes", "4", "--seed", "4",
               "--report-every", "1", "--save", "av.pt", "--log", "av.csv")
    assert t.returncode == 0, t.stderr[-2000:]


def test_evaluate_search_and_its_refusals(pkg, tmp_path):
    train_afterstate(tmp_path, "cpu", 64)
    common = ("evaluate.py", "--model", "av.pt", "--num-envs", "48", "--episodes", "1", "--steps-per-launch", "16", "--seed", "5")
    greedy, searched = script(tmp_path, "cpu", *common, "--fused"), script(tmp_path, "cpu", *common, "--fused", "--search")
    assert greedy.returncode == 0 and searched.returncode == 0, greedy.stderr[-2000:] + searched.stderr[-2000:]
    g, s = last_json(greedy), last_json(searched)
    assert g["search"] == 0 and s["search"] == 1 and set(g) == set(s)
    assert s["agent"] == "afterstate" and s["fused"] is True and s["games"] >= 48 and s["epsilon"] == 0.0
    assert sum(s["max_tile_hist"].values()) == s["games"] and 0.0 < s["valid_move_frac"] <= 1.0
    assert (g["env_steps"], g["mean_score"]) != (s["env_steps"], s["mean_score"]), "the searched player played the greedy games"
    # --search without --fused
    bad = script(tmp_path, "cpu", *common, "--search")
    assert bad.returncode != 0 and "--search needs --fused" in bad.stderr
    bad = script(tmp_path, "cpu", *common, "--search", "--policy", "reference")
    assert bad.returncode != 0 and "--search needs --fused" in bad.stderr
    # --search on files of other kinds: refused with the kind the file holds
    torch.save(pkg.BatchedQLearningAgent(6, capacity_log2=12, device="cpu", placement="plain").state_dict(), tmp_path / "h.pt")
    torch.save(pkg.BatchedRowTupleAgent(6, device="cpu").state_dict(), tmp_path / "rowtuple.pt")
    torch.save(pkg.BatchedLineTupleAgent(6, device="cpu").state_dict(), tmp_path / "linetuple.pt")
    for name, kind in (("h.pt", "hash_table"), ("rowtuple.pt", "row_tuple"), ("linetuple.pt", "line_tuple")):
        bad = script(tmp_path, "cpu", "evaluate.py", "--model", name, "--num-envs", "48", "--episodes", "1", "--fused", "--search")
        assert bad.returncode != 0 and "--search needs a file of kind line_afterstate or ntuple6_afterstate" in bad.stderr, name
        assert f"holds kind {kind}" in bad.stderr and "Traceback" not in bad.stderr, name


@pytest.mark.gpu
def test_evaluate_search_on_the_device(pkg, tmp_path):
    train_afterstate(tmp_path, "cuda", 256)
    common = ("evaluate.py", "--model", "av.pt", "--num-envs", "256", "--episodes", "1", "--seed", "5", "--fused")
    greedy, searched = script(tmp_path, "cuda", *common), script(tmp_path, "cuda", *common, "--search")
    assert greedy.returncode == 0 and searched.returncode == 0, greedy.stderr[-2000:] + searched.stderr[-2000:]
    g, s = last_json(greedy), last_json(searched)
    assert g["search"] == 0 and s["search"] == 1 and s["agent"] == "afterstate" and s["games"] >= 256
    assert sum(s["max_tile_hist"].values()) == s["games"]
    host = last_json(script(tmp_path, "cpu", *common, "--search"))                       # the same file on the twin: the same games
    for key in ("games", "env_steps", "mean_score", "max_tile_hist", "valid_move_frac"):
        assert host[key] == s[key], key
