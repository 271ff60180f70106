#!/usr/bin/env python3
"""The staged 6-tuple network (q2048_nts_*, a table of weights per largest-tile stage) measured beside the plain network
of the same build.  Every step that uses the GPU is a child process under its own `timeout`; the steps are chained, and
the first one that fails ends the run.

  step_time   q2048_nts_fused_rollout / q2048_nts_play_rollout with stages == 0 and with the threshold (11,) = the tile
              2048, and in the same process q2048_nt_fused_rollout / q2048_nt_play_rollout, at 65,536 and 1,048,576
              boards: every learner trains --warm steps at that size first, then five alternating 64-step regions each
              by HIP events; the median per step and the ratios nts / nt.  Then q2048_nts_promote: five calls from a
              trained stage into a zeroed one, the median against the 768 MiB a call moves at most (two tables read,
              one written)                                                         -> r18_stages_step_time.jsonl
  strength    the command of README's network row, `train.py --agent ntuple --num-envs 65536 --episodes 40
              --eval-every 5 --seed 0`, plain and with `--stage-tiles 2048`; then the plain 40-epoch file trained 40
              more epochs, plain and split by `--resume ... --stage-tiles 2048`; then `evaluate.py --fused`, `--fused
              --search` and `--fused --search --search-depth 2` at --num-envs-eval envs on each of the four files
                                              -> r18_stages_strength.jsonl, r18_stages_train_<name>{.log,_eval.jsonl}
    python tools/exp_stages.py --out profiles
`--device cpu --envs 2048 --num-envs 256 --num-envs-eval 64 --episodes 4 --eval-every 2 --warm 50 --regions 2 --region 4`
rehearses the script on the CPU twin (host clock; its times say nothing about the GPU).  One seed: the strength figures
are one run each."""
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
p.add_argument("--out", default="profiles", help="directory of the r18_stages_* files")
p.add_argument("--steps", nargs="*", default=["step_time", "strength"])
p.add_argument("--envs", type=int, nargs="*", default=[65536, 1 << 20], help="batch sizes of step_time")
p.add_argument("--region", type=int, default=64, help="steps per timed region")
p.add_argument("--regions", type=int, default=5)
p.add_argument("--warm", type=int, default=300, help="training steps before the regions")
p.add_argument("--num-envs", type=int, default=65536, help="strength: train.py --num-envs")
p.add_argument("--num-envs-eval", type=int, default=16384, help="strength: evaluate.py --num-envs")
p.add_argument("--episodes", type=int, default=40)
p.add_argument("--eval-every", type=int, default=5)
p.add_argument("--eval-episodes", type=int, default=2, help="strength: evaluate.py --episodes")
p.add_argument("--stage-tiles", default="2048")
p.add_argument("--depths", type=int, nargs="*", default=[0, 1, 2], help="strength: 0 = greedy, 1, 2 = --search-depth")
p.add_argument("--seed", type=int, default=0, help="strength: train.py --seed")
p.add_argument("--limit", type=int, default=420, help="seconds a child process (one script of strength) may take")
p.add_argument("--child", default="", help="(internal) the step this process runs itself")
p.add_argument("--models", default="models", help="where the saved learners go (relative to the repository)")
args = p.parse_args()
out = lambda name: os.path.join(os.path.abspath(args.out), name)  # noqa: E731


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

    def learner(tiles, zero_spec=False):
        agent = pkg.BatchedNTupleAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.1, seed=3, device=dev,
                                       stage_tiles=tiles)
        if zero_spec:                   # the staged entry points with stages == 0: the plain network through q2048_nts_*
            agent._stages = 0
        return agent

    names = ("nt", "nts0", "nts11")
    with open(out("r18_stages_step_time.jsonl"), "w") as fh:
        for B in args.envs:
            learners = {}
            for name, agent in (("nt", learner(())), ("nts0", learner((2048,), True)), ("nts11", learner((2048,)))):
                env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                agent.fused_rollout(env, args.warm)                 # trained weights, mid-game boards
                play_env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                play_env.load_state_dict(env.state_dict())
                learners[name] = (agent, env, play_env)
            cases = {f"{n}_{k}": [] for k in ("fused", "play") for n in names}
            for name, (agent, env, play_env) in learners.items():   # one untimed region each: first-launch costs
                agent.fused_rollout(env, args.region)
                agent.play_rollout(play_env, args.region)
            for r in range(args.regions):                           # alternating, the order turned round every region
                order = names if r % 2 == 0 else names[::-1]
                for name in order:
                    agent, env, _ = learners[name]
                    cases[f"{name}_fused"].append(timed(lambda: agent.fused_rollout(env, args.region)))
                for name in order:
                    agent, _, play_env = learners[name]
                    cases[f"{name}_play"].append(timed(lambda: agent.play_rollout(play_env, args.region)))
            us = {k: statistics.median(v) * 1e3 / args.region for k, v in cases.items()}
            staged = learners["nts11"][0]
            line = {"case": "stages_step_time", "device": str(dev), "envs": B, "steps_per_region": args.region,
                    "regions": args.regions, "warm_steps": args.warm,
                    **{f"{k}_ms": [round(x, 3) for x in v] for k, v in cases.items()},
                    **{f"{k}_us_per_step": round(v, 3) for k, v in us.items()},
                    **{f"{n}_over_nt_{k}": round(us[f"{n}_{k}"] / us[f"nt_{k}"], 3) for n in names[1:] for k in ("fused", "play")},
                    "nts11_weights_touched": [int(torch.count_nonzero(staged.weights[k]).item()) for k in range(2)]}
            fh.write(json.dumps(line) + "\n")
            fh.flush()
            print(json.dumps(line), flush=True)
            if B == args.envs[0]:                                   # promotion: a trained stage into a zeroed one
                agent = learners["nts11"][0]
                ms, counts = [], []
                for _ in range(args.regions):
                    agent.weights[1].zero_()
                    if on_gpu:
                        torch.cuda.synchronize()
                    ms.append(timed(lambda: counts.append(agent.promote())))
                again = timed(lambda: counts.append(agent.promote()))           # nothing left to copy: two tables read
                med = statistics.median(ms)
                line = {"case": "stages_promote", "device": str(dev), "calls_ms": [round(x, 3) for x in ms],
                        "median_ms": round(med, 3), "entries_copied": counts[0][0], "bytes_moved_at_most": 3 << 28,
                        "gb_per_s_at_most": round((3 << 28) / med / 1e6, 1), "nothing_to_copy_ms": round(again, 3),
                        "nothing_to_copy_count": counts[-1][0]}
                fh.write(json.dumps(line) + "\n")
                fh.flush()
                print(json.dumps(line), flush=True)
            del learners


def script(name, *a, log=None):
    cmd = [sys.executable, os.path.join(REPO, name), "--device", args.device.split(":")[0], *a]
    print(" ".join(cmd), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(args.limit)] + cmd, capture_output=True, text=True, cwd=REPO)
    if log:
        with open(log, "w") as fh:
            fh.write(r.stdout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(r.returncode)                   # a fault, an abort or a time limit: nothing more is started
    return r.stdout


def strength():
    n, e = args.num_envs, args.episodes
    model = lambda name: os.path.join(args.models, f"stages_{name}.pt")      # noqa: E731
    train = ("train.py", "--agent", "ntuple", "--num-envs", str(n), "--seed", str(args.seed), "--eval-every", str(args.eval_every))
    tiles = ("--stage-tiles", args.stage_tiles)
    runs = [(f"plain_{e}", ("--episodes", str(e))), (f"staged_{e}", ("--episodes", str(e), *tiles)),
            (f"plain_{2 * e}", ("--episodes", str(2 * e), "--resume", model(f"plain_{e}"))),
            (f"split_{2 * e}", ("--episodes", str(2 * e), "--resume", model(f"plain_{e}"), *tiles))]
    for name, extra in runs:
        tag = f"r18_stages_train_{name}"
        script(*train, *extra, "--eval-log", out(f"{tag}_eval.jsonl"), "--log", os.devnull, "--save", model(name),
               log=out(f"{tag}.log"))
    with open(out("r18_stages_strength.jsonl"), "w") as fh:
        for depth in args.depths:                                   # the cheap players of every file first
            for name, _ in runs:
                extra = () if depth == 0 else ("--search", "--search-depth", str(depth))
                text = script("evaluate.py", "--model", model(name), "--num-envs", str(args.num_envs_eval), "--episodes",
                              str(args.eval_episodes), "--seed", str(args.seed), "--fused", *extra)
                line = {"case": "stages_strength", "file": name, **json.loads(text.strip().splitlines()[-1])}
                fh.write(json.dumps(line) + "\n")
                fh.flush()
                print(json.dumps({k: line[k] for k in ("file", "search", "stage_tiles", "games", "mean_score")}), flush=True)


if args.child:
    {"step_time": step_time, "strength": strength}[args.child]()
    raise SystemExit(0)

os.makedirs(args.out, exist_ok=True)
os.makedirs(os.path.join(REPO, args.models), exist_ok=True)
for step in args.steps:
    limit = args.limit if step == "step_time" else args.limit * 16        # strength: sixteen scripts, each under --limit
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", step] + sys.argv[1:]
    t0 = time.time()
    rc = subprocess.run(cmd).returncode
    print(f"[{step}] exit {rc} after {time.time() - t0:.1f} s", flush=True)
    if rc != 0:                                      # a fault, an abort or a time limit: nothing more is started
        raise SystemExit(rc)
