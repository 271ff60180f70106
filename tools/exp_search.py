#!/usr/bin/env python3
"""The one-level expectimax player (q2048_{av,nt}_search_play_rollout) measured beside the greedy player of the same
build, for both afterstate families.  Every step that uses the GPU is a child process under its own `timeout`; the
steps are chained, and the first one that fails ends the run.

  step_time   per family and batch size (4,096, 65,536 and 1,048,576 boards): the learner trains --warm steps at that
              size (trained weights, mid-game boards), then five alternating 64-step regions of the greedy and of the
              searched player, each by HIP events, from the same boards; the median per step, the ratio searched /
              greedy, and beside it the count the ratio is held against: a searched step makes (live chance nodes + 1)
              evaluations where a greedy step makes one -- the nodes are counted on a sample of the timed boards
                                                                                  -> r15_search_step_time.jsonl
  strength    `train.py --agent <afterstate|ntuple> --num-envs 65536 --episodes 40 --seed 0 --save` (the commands behind
              r13_av_train_65536x40 and r14_nt_train_65536x40), then `evaluate.py --fused` and `evaluate.py --fused
              --search` on that one file with the same --seed, --num-envs and --episodes
                                                                                  -> r15_search_strength.jsonl
    python tools/exp_search.py --out profiles
`--device cpu --envs 256 --num-envs 256 --episodes 4 --warm 50 --regions 2 --region 4` rehearses the script on the CPU
twin (host clock; its times say nothing about the GPU).

`--depth 2` measures the TWO-level player (q2048_{av,nt}_search_play_rollout_depth) beside the one-level player of the
same build, whose kernel no later change has touched:
  step_time   per family and batch size (`--envs 4096 65536`; 1,048,576 is a count, not a timing): the same training,
              then alternating regions of the depth-1 (--region steps) and the depth-2 player (--region2 steps, 8) from
              the same boards; the medians per step, their ratio, and the count it is held against: leaf evaluations
              per depth-2 step (over the level-one nodes of a board, the sum of THEIR live nodes, counted on --sample2
              of the timed boards) over the live nodes of a depth-1 step; and both rates, leaf evaluations per second
              beside the depth-1 player's node evaluations per second         -> r17_search2_step_time.jsonl
  strength    the same two training commands, then `evaluate.py --fused`, `--fused --search` and `--fused --search
              --search-depth 2` on that one file with the same seed (pass --num-envs-eval 16384).  Two children: the
              first trains and plays the greedy and the one-level player; the time limit of the second, the depth-2
              player, is SIZED from what was measured -- the steps per env of the one-level games just played (doubled:
              a stronger player's games are longer) times the depth-2 step time of r17_search2_step_time.jsonl scaled
              to the batch, times three, plus a minute -- so step_time has to have run
                                                                                  -> r17_search2_strength.jsonl
    python tools/exp_search.py --depth 2 --steps step_time --envs 4096 65536
    python tools/exp_search.py --depth 2 --steps strength --num-envs-eval 16384"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

p = argparse.ArgumentParser()
p.add_argument("--device", default="cuda:0")
p.add_argument("--out", default="profiles", help="directory of the r15_search_* files")
p.add_argument("--steps", nargs="*", default=["step_time", "strength"])
p.add_argument("--families", nargs="*", default=["av", "nt"])
p.add_argument("--envs", type=int, nargs="*", default=[4096, 65536, 1 << 20], help="batch sizes of step_time")
p.add_argument("--region", type=int, default=64, help="steps per timed region")
p.add_argument("--regions", type=int, default=5)
p.add_argument("--warm", type=int, default=300, help="training steps before the regions")
p.add_argument("--sample", type=int, default=4096, help="boards on which the live nodes are counted")
p.add_argument("--num-envs", type=int, default=65536, help="strength: --num-envs of train.py and evaluate.py")
p.add_argument("--episodes", type=int, default=40, help="strength: train.py --episodes")
p.add_argument("--eval-episodes", type=int, default=2, help="strength: evaluate.py --episodes")
p.add_argument("--seed", type=int, default=0, help="strength: train.py --seed")
p.add_argument("--limit", type=int, default=420, help="seconds a child process may take")
p.add_argument("--child", default="", help="(internal) the step this process runs itself")
p.add_argument("--models", default="models", help="where the saved learners go (relative to the repository)")
p.add_argument("--depth", type=int, choices=[1, 2], default=1, help="2: the two-level player beside the one-level one (r17_search2_*)")
p.add_argument("--region2", type=int, default=8, help="--depth 2: steps per timed region of the depth-2 player")
p.add_argument("--sample2", type=int, default=512, help="--depth 2: boards on which the leaf evaluations are counted")
p.add_argument("--num-envs-eval", type=int, default=0, help="strength: evaluate.py --num-envs (0: --num-envs)")
args = p.parse_args()
out = lambda name: os.path.join(os.path.abspath(args.out), name)  # noqa: E731
AGENT = {"av": "afterstate", "nt": "ntuple"}
STEP_TIME2, STRENGTH2 = "r17_search2_step_time.jsonl", "r17_search2_strength.jsonl"


def live_nodes(boards):
    """Chance nodes of one searched step, per board: over the moves that change the board, 2 x the empty cells of the
    moved board.  numpy uint8 [B, 16] -> int64 [B].  (A slide keeps the tiles and a merge removes one, so the moved
    board has the empty cells of the board plus one per merge.)"""
    import numpy as np

    b = boards.reshape(-1, 4, 4)
    total = np.zeros(len(b), np.int64)
    for lines in (b, b[:, :, ::-1], b.transpose(0, 2, 1), b.transpose(0, 2, 1)[:, :, ::-1]):     # left, right, up, down
        merges, changed = np.zeros(len(b), np.int64), np.zeros(len(b), bool)
        for r in range(4):
            line = lines[:, r, :]
            packed = np.zeros_like(line)
            fill = np.zeros(len(b), np.int64)
            for c in range(4):                                       # compress towards cell 0
                put = line[:, c] != 0
                packed[put, fill[put]] = line[put, c]
                fill += put
            changed |= (packed != line).any(axis=1)
            c, rows = np.zeros(len(b), np.int64), np.arange(len(b))
            for _ in range(3):                                       # one left-to-right pass, a merged tile merges no more
                at = np.minimum(c, 2)
                pair = (c < 3) & (packed[rows, at] != 0) & (packed[rows, at] == packed[rows, at + 1])
                merges += pair
                c += np.where(pair, 2, 1)
        changed |= merges > 0
        empties = (b.reshape(len(b), 16) == 0).sum(axis=1) + merges
        total += np.where(changed, 2 * empties, 0)
    return total


def chance_nodes(boards):
    """The level-one nodes of a batch (which board each belongs to is not kept): for every move that changes a board,
    the moved board with a 2 and with a 4 in every empty cell.  numpy uint8 [B, 16] -> uint8 [nodes, 16].  For counting
    only: a merged tile is its exponent + 1 without a cap."""
    import numpy as np

    def moved_left(lines):
        n, rows = len(lines), np.arange(len(lines))
        packed, fill = np.zeros_like(lines), np.zeros(len(lines), np.int64)
        for c in range(4):                                           # compress towards cell 0
            put = lines[:, c] != 0
            packed[put, fill[put]] = lines[put, c]
            fill += put
        res, w, c = np.zeros_like(lines), np.zeros(n, np.int64), np.zeros(n, np.int64)
        for _ in range(4):                                           # one left-to-right pass, a merged tile merges no more
            at, nxt = np.minimum(c, 3), np.minimum(c + 1, 3)
            v = packed[rows, at]
            pair = (c < 3) & (v != 0) & (v == packed[rows, nxt])
            sel = (c < 4) & (v != 0)
            res[rows[sel], w[sel]] = np.where(pair, v + 1, v)[sel]
            w += sel
            c += np.where(pair, 2, 1)
        return res

    b = np.ascontiguousarray(boards, dtype=np.uint8).reshape(-1, 4, 4)
    nodes = []
    for k in range(4):                                               # left, right, up, down
        view = b if k < 2 else b.transpose(0, 2, 1)
        view = view[:, :, ::-1] if k & 1 else view
        m = moved_left(np.ascontiguousarray(view).reshape(-1, 4)).reshape(-1, 4, 4)
        m = m[:, :, ::-1] if k & 1 else m
        m = np.ascontiguousarray(m if k < 2 else m.transpose(0, 2, 1)).reshape(-1, 16)
        m = m[(m != b.reshape(-1, 16)).any(axis=1)]
        i, j = np.nonzero(m == 0)
        for tile in (1, 2):
            n = m[i].copy()
            n[np.arange(len(i)), j] = tile
            nodes.append(n)
    return np.concatenate(nodes) if nodes else np.zeros((0, 16), np.uint8)


def step_time2():
    """--depth 2: the depth-2 player beside the depth-1 player of the same build."""
    import importlib

    import torch

    sys.path.insert(0, REPO)
    pkg = importlib.import_module("2048_q-learning_amd")
    dev = torch.device(args.device)
    on_gpu = dev.type == "cuda"
    if on_gpu:
        torch.cuda.set_device(dev)

    def timed(fn):
        if not on_gpu:
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def counts(boards):
        """(live nodes of a depth-1 step, leaf evaluations of a depth-2 step), means per board of the sample"""
        s = boards[:args.sample2].cpu().numpy()
        return float(live_nodes(s).mean()), float(live_nodes(chance_nodes(s)).sum()) / len(s)

    classes = {"av": pkg.BatchedAfterstateAgent, "nt": pkg.BatchedNTupleAgent}
    with open(out(STEP_TIME2), "w") as fh:
        for fam in args.families:
            for B in args.envs:
                agent = classes[fam](100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.1, seed=3, device=dev)
                env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                agent.fused_rollout(env, args.warm)                  # trained weights, mid-game boards
                start = env.state_dict()
                envs = {}
                for k in ("search", "search2"):
                    envs[k] = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                    envs[k].load_state_dict(start)
                play = {"search": lambda e, n: agent.search_rollout(e, n), "search2": lambda e, n: agent.search_rollout(e, n, depth=2)}
                region = {"search": args.region, "search2": args.region2}
                w = agent.weights.cpu()
                for k in play:                                       # one untimed launch each: first-launch costs
                    play[k](envs[k], 1)
                cases, nodes, leaves = {"search": [], "search2": []}, [], []
                for r in range(args.regions):                        # alternating, the order turned round every region
                    nodes.append(counts(envs["search"].boards)[0])
                    leaves.append(counts(envs["search2"].boards)[1])
                    for k in (("search", "search2") if r % 2 == 0 else ("search2", "search")):
                        cases[k].append(timed(lambda: play[k](envs[k], region[k])))
                nodes.append(counts(envs["search"].boards)[0])
                leaves.append(counts(envs["search2"].boards)[1])
                assert torch.equal(w.view(torch.int32), agent.weights.cpu().view(torch.int32)), f"{fam}: a player wrote"
                us = {k: statistics.median(v) * 1e3 / region[k] for k, v in cases.items()}
                mean_nodes, mean_leaves = sum(nodes) / len(nodes), sum(leaves) / len(leaves)
                node_rate, leaf_rate = B * mean_nodes / us["search"] * 1e6, B * mean_leaves / us["search2"] * 1e6
                line = {"case": "search2_step_time", "family": fam, "device": str(dev), "envs": B,
                        "steps_per_region": region, "regions": args.regions, "warm_steps": args.warm,
                        **{f"{k}_ms": [round(x, 3) for x in v] for k, v in cases.items()},
                        **{f"{k}_us_per_step": round(v, 3) for k, v in us.items()},
                        "search2_over_search": round(us["search2"] / us["search"], 3),
                        "mean_live_nodes": round(mean_nodes, 3), "mean_leaf_evaluations": round(mean_leaves, 3),
                        "count_ratio": round(mean_leaves / mean_nodes, 3),
                        "ratio_over_count": round(us["search2"] / us["search"] / (mean_leaves / mean_nodes), 4),
                        "search_node_evaluations_per_s": round(node_rate, 1),
                        "search2_leaf_evaluations_per_s": round(leaf_rate, 1),
                        "leaf_rate_over_node_rate": round(leaf_rate / node_rate, 4),
                        "search2_env_steps_per_s": round(B / us["search2"] * 1e6, 1),
                        "counted_on": min(args.sample2, B)}
                fh.write(json.dumps(line) + "\n")
                fh.flush()
                print(json.dumps(line), flush=True)
                del agent, env, envs, w


def step_time():
    import importlib

    import torch

    sys.path.insert(0, REPO)
    pkg = importlib.import_module("2048_q-learning_amd")
    dev = torch.device(args.device)
    on_gpu = dev.type == "cuda"
    if on_gpu:
        torch.cuda.set_device(dev)

    def timed(fn):
        if not on_gpu:
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    classes = {"av": pkg.BatchedAfterstateAgent, "nt": pkg.BatchedNTupleAgent}
    with open(out("r15_search_step_time.jsonl"), "w") as fh:
        for fam in args.families:
            for B in args.envs:
                agent = classes[fam](100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.1, seed=3, device=dev)
                env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                agent.fused_rollout(env, args.warm)                  # trained weights, mid-game boards
                start = env.state_dict()
                envs = {}
                for k in ("greedy", "search"):
                    envs[k] = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                    envs[k].load_state_dict(start)
                play = {"greedy": agent.play_rollout, "search": agent.search_rollout}
                w = agent.weights.cpu()
                for k in play:                                       # one untimed launch each: first-launch costs
                    play[k](envs[k], 1)
                cases, nodes = {"greedy": [], "search": []}, []
                for r in range(args.regions):                        # alternating, the order turned round every region
                    nodes.append(live_nodes(envs["search"].boards[:args.sample].cpu().numpy()))
                    for k in (("greedy", "search") if r % 2 == 0 else ("search", "greedy")):
                        cases[k].append(timed(lambda: play[k](envs[k], args.region)))
                nodes.append(live_nodes(envs["search"].boards[:args.sample].cpu().numpy()))
                assert torch.equal(w.view(torch.int32), agent.weights.cpu().view(torch.int32)), f"{fam}: a player wrote"
                us = {k: statistics.median(v) * 1e3 / args.region for k, v in cases.items()}
                mean_nodes = float(sum(n.mean() for n in nodes) / len(nodes))
                st = agent.play_stats()
                line = {"case": "search_step_time", "family": fam, "device": str(dev), "envs": B,
                        "steps_per_region": args.region, "regions": args.regions, "warm_steps": args.warm,
                        **{f"{k}_ms": [round(x, 3) for x in v] for k, v in cases.items()},
                        **{f"{k}_us_per_step": round(v, 3) for k, v in us.items()},
                        "search_over_greedy": round(us["search"] / us["greedy"], 3),
                        "mean_live_nodes": round(mean_nodes, 3), "evaluations_per_searched_step": round(mean_nodes + 1.0, 3),
                        "ratio_over_count": round(us["search"] / us["greedy"] / (mean_nodes + 1.0), 4),
                        "search_env_steps_per_s": round(B / us["search"] * 1e6, 1),
                        "search_node_evaluations_per_s": round(B * mean_nodes / us["search"] * 1e6, 1),
                        "nodes_sampled_on": min(args.sample, B), "play_valid_move_frac": round(st["valid_moves"] / max(st["steps"], 1), 6)}
                fh.write(json.dumps(line) + "\n")
                fh.flush()
                print(json.dumps(line), flush=True)
                del agent, env, envs, w


def script(name, *a, log=None, limit=None):
    cmd = [sys.executable, os.path.join(REPO, name), "--device", args.device.split(":")[0], *a]
    print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=limit or args.limit)
    if log:
        with open(log, "w") as fh:
            fh.write(r.stdout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(r.returncode)
    return r.stdout


def strength():
    n, e = args.num_envs, args.episodes
    with open(out("r15_search_strength.jsonl"), "w") as fh:
        for fam in args.families:
            model = os.path.join(args.models, f"{fam}_{n}x{e}.pt")
            script("train.py", "--agent", AGENT[fam], "--num-envs", str(n), "--episodes", str(e), "--seed", str(args.seed),
                   "--save", model, "--log", os.devnull, log=out(f"r15_search_train_{fam}_{n}x{e}.log"))
            common = ("evaluate.py", "--model", model, "--num-envs", str(n), "--episodes", str(args.eval_episodes), "--fused")
            for extra in ((), ("--search",)):
                line = json.loads(script(*common, *extra).strip().splitlines()[-1])
                fh.write(json.dumps({"case": "search_strength", "family": fam, **line}) + "\n")
                fh.flush()
                print(json.dumps(line), flush=True)


def eval_common(fam):
    n, e = args.num_envs, args.episodes
    model = os.path.join(args.models, f"{fam}_{n}x{e}.pt")
    return model, ("evaluate.py", "--model", model, "--num-envs", str(args.num_envs_eval or n), "--episodes",
                   str(args.eval_episodes), "--fused")


def strength2_shallow():
    """--depth 2, first child: train, then the greedy and the one-level player -> the first lines of r17_search2_strength"""
    n, e = args.num_envs, args.episodes
    with open(out(STRENGTH2), "w") as fh:
        for fam in args.families:
            model, common = eval_common(fam)
            script("train.py", "--agent", AGENT[fam], "--num-envs", str(n), "--episodes", str(e), "--seed", str(args.seed),
                   "--save", model, "--log", os.devnull, log=out(f"r17_search2_train_{fam}_{n}x{e}.log"))
            for extra in ((), ("--search",)):
                line = json.loads(script(*common, *extra).strip().splitlines()[-1])
                fh.write(json.dumps({"case": "search2_strength", "family": fam, **line}) + "\n")
                fh.flush()
                print(json.dumps(line), flush=True)


def strength2_limits():
    """Seconds the depth-2 player of each family may take, from what was measured: (steps per env of the one-level games,
    doubled) x (the depth-2 step time at the largest timed batch, scaled to the evaluated batch) x 3 + 60."""
    with open(out(STEP_TIME2)) as fh:
        timed = [json.loads(x) for x in fh if x.strip()]
    with open(out(STRENGTH2)) as fh:
        played = [json.loads(x) for x in fh if x.strip()]
    limits = {}
    for fam in args.families:
        step = max((x for x in timed if x["family"] == fam), key=lambda x: x["envs"])
        one = next(x for x in played if x["family"] == fam and x["search"] == 1)
        steps_per_env = 2.0 * one["env_steps"] / one["envs"]
        us_per_step = step["search2_us_per_step"] * max(one["envs"] / step["envs"], 1.0 / 16.0)   # (a small batch does not scale down)
        limits[fam] = 60.0 + 3.0 * steps_per_env * us_per_step * 1e-6
    return limits


def strength2_deep():
    """--depth 2, second child: the depth-2 player on the saved files, each family under its own sized limit (the parent
    gives this process their sum)."""
    limits = strength2_limits()
    with open(out(STRENGTH2), "a") as fh:
        for fam in args.families:
            _, common = eval_common(fam)
            t0 = time.time()
            line = json.loads(script(*common, "--search", "--search-depth", "2", limit=limits[fam]).strip().splitlines()[-1])
            line["time_limit_s"], line["wall_s"] = round(limits[fam], 1), round(time.time() - t0, 1)
            fh.write(json.dumps({"case": "search2_strength", "family": fam, **line}) + "\n")
            fh.flush()
            print(json.dumps(line), flush=True)


if args.child:
    {"step_time": step_time, "strength": strength, "step_time2": step_time2, "strength2_shallow": strength2_shallow,
     "strength2_deep": strength2_deep}[args.child]()
    raise SystemExit(0)

os.makedirs(args.out, exist_ok=True)
os.makedirs(os.path.join(REPO, args.models), exist_ok=True)
for step in args.steps:
    children = [step] if args.depth == 1 else {"step_time": ["step_time2"], "strength": ["strength2_shallow", "strength2_deep"]}[step]
    for child in children:
        limit = args.limit
        if child == "strength2_deep":                # sized from the step time and the one-level games measured before it
            limit = int(sum(strength2_limits().values())) + 30
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", child] + sys.argv[1:]
        t0 = time.time()
        rc = subprocess.run(cmd).returncode
        print(f"[{child}] exit {rc} (limit {limit} s) after {time.time() - t0:.1f} s", flush=True)
        if rc != 0:                                  # a fault, an abort or a time limit: nothing more is started
            raise SystemExit(rc)
