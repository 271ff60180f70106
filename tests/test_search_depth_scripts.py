"""`evaluate.py --search --search-depth`: the two-level expectimax player through the script, on a tiny file of each
afterstate family saved by `train.py`, and its refusals -- without `--search`, on a file of another kind.  As
subprocesses on the CPU twin, and once per family on the GPU.  The helpers are those of the row-tuple learner's and of
the one-level player's script tests."""
import pytest
import torch

import test_row_tuple_player as P
import test_search_scripts as SS

script, last_json = P.script, SS.last_json
AGENTS = {"av": "afterstate", "nt": "ntuple"}
ENVS = 3             # a searched player lasts a thousand steps even on these files: the twin walks every leaf serially
GAMES = ("games", "env_steps", "mean_score", "max_tile_hist", "valid_move_frac")


def train(tmp_path, device, fam, envs):
    t = script(tmp_path, device, "train.py", "--agent", AGENTS[fam], "--num-envs", str(envs), "--episodes", "4", "--seed", "4",
               "--report-every", "1", "--save", f"{fam}.pt", "--log", f"{fam}.csv")
    assert t.returncode == 0, t.stderr[-2000:]


def evaluate(tmp_path, device, fam, envs, *extra):
    return script(tmp_path, device, "evaluate.py", "--model", f"{fam}.pt", "--num-envs", str(envs), "--episodes", "1",
                  "--steps-per-launch", "16", "--seed", "5", *extra)


@pytest.mark.parametrize("fam", ["av", "nt"])
def test_evaluate_search_depth(pkg, tmp_path, fam):
    train(tmp_path, "cpu", fam, 64)
    runs = [evaluate(tmp_path, "cpu", fam, ENVS, "--fused", *extra)
            for extra in ((), ("--search",), ("--search", "--search-depth", "1"), ("--search", "--search-depth", "2"))]
    assert all(r.returncode == 0 for r in runs), "".join(r.stderr[-2000:] for r in runs)
    greedy, one, one_again, two = (last_json(r) for r in runs)
    assert [greedy["search"], one["search"], one_again["search"], two["search"]] == [0, 1, 1, 2]
    assert set(greedy) == set(one) == set(two), "the set of keys is unchanged"
    assert two["agent"] == AGENTS[fam] and two["fused"] is True and two["games"] >= ENVS and two["epsilon"] == 0.0
    assert sum(two["max_tile_hist"].values()) == two["games"] and 0.0 < two["valid_move_frac"] <= 1.0
    assert all(one[k] == one_again[k] for k in GAMES), "--search alone is depth 1"
    assert any(one[k] != two[k] for k in GAMES), "the depth-2 player played the depth-1 games"


def test_search_depth_refusals(pkg, tmp_path):
    train(tmp_path, "cpu", "av", 64)
    for extra in (("--fused",), (), ("--policy", "reference")):
        bad = evaluate(tmp_path, "cpu", "av", 24, "--search-depth", "2", *extra)
        assert bad.returncode != 0 and "--search-depth needs --search" in bad.stderr and "Traceback" not in bad.stderr
    bad = evaluate(tmp_path, "cpu", "av", 24, "--search", "--search-depth", "2")
    assert bad.returncode != 0 and "--search needs --fused" in bad.stderr
    bad = evaluate(tmp_path, "cpu", "av", 24, "--fused", "--search", "--search-depth", "3")
    assert bad.returncode != 0 and "--search-depth" in bad.stderr and "Traceback" not in bad.stderr
    # files of other kinds: refused as without a depth, with the kind the file holds
    torch.save(pkg.BatchedQLearningAgent(6, capacity_log2=12, device="cpu", placement="plain").state_dict(), tmp_path / "h.pt")
    torch.save(pkg.BatchedRowTupleAgent(6, device="cpu").state_dict(), tmp_path / "rowtuple.pt")
    for name, kind in (("h.pt", "hash_table"), ("rowtuple.pt", "row_tuple")):
        bad = script(tmp_path, "cpu", "evaluate.py", "--model", name, "--num-envs", "24", "--episodes", "1", "--fused",
                     "--search", "--search-depth", "2")
        assert bad.returncode != 0 and "--search needs a file of kind line_afterstate or ntuple6_afterstate" in bad.stderr, name
        assert f"holds kind {kind}" in bad.stderr and "Traceback" not in bad.stderr, name


@pytest.mark.gpu
@pytest.mark.parametrize("fam", ["av", "nt"])
def test_evaluate_search_depth_on_the_device(pkg, tmp_path, fam):
    """The file is trained on the CPU twin (a learning run on the device is not reproducible run to run); the device and
    the twin then play the same games from it at depth 2."""
    train(tmp_path, "cpu", fam, 64)
    one = last_json(evaluate(tmp_path, "cuda", fam, ENVS, "--fused", "--search"))
    dev = evaluate(tmp_path, "cuda", fam, ENVS, "--fused", "--search", "--search-depth", "2")
    assert dev.returncode == 0, dev.stderr[-2000:]
    d = last_json(dev)
    assert d["search"] == 2 and one["search"] == 1 and d["agent"] == AGENTS[fam] and d["games"] >= ENVS
    assert sum(d["max_tile_hist"].values()) == d["games"]
    assert any(one[k] != d[k] for k in GAMES), "the depth-2 player played the depth-1 games"
    host = last_json(evaluate(tmp_path, "cpu", fam, ENVS, "--fused", "--search", "--search-depth", "2"))
    for key in GAMES:
        assert host[key] == d[key], key
