#!/usr/bin/env python3
"""The line-tuple learner (rows and columns as features, 8 MiB of weights) measured beside the row-tuple learner
(rows only, 4 MiB), on one build.  Every step that uses the GPU is a child process under its own `timeout`; the steps
are chained, and the first one that fails ends the run.

  step_time   q2048_lt_fused_rollout / q2048_lt_play_rollout and, in the same process, q2048_rt_fused_rollout /
              q2048_rt_play_rollout at 65,536 and 1,048,576 boards: both learners train --warm steps at that size
              first (trained weights, mid-game boards), then five alternating 64-step regions each by HIP events;
              the median per step and the ratio lt / rt                      -> r12_lt_step_time.jsonl
  learn       `train.py --agent line-tuple --num-envs 65536 --episodes 40 --eval-every 5` (the command behind
              r11_rt_train_65536x40_eval.jsonl, with the other agent) and `evaluate.py --fused` on the saved file
                                                     -> r12_lt_train_65536x40{.log,.csv,_eval.jsonl}, r12_lt_evaluate_65536x40.jsonl
  promote     the row-tuple run again (its curve is the cross-check against r11), its file resumed as line-tuple for
              40 more epochs, and `evaluate.py --fused` on both files
                                                     -> r12_rt_train_65536x40_eval.jsonl, r12_lt_promoted_65536x80{.log,.csv,_eval.jsonl},
                                                        r12_lt_promoted_evaluate.jsonl
    python tools/exp_line_tuple.py --out profiles
`--device cpu --envs 2048 --num-envs 256 --episodes 4 --eval-every 2` rehearses the script on the CPU twin (host clock;
its times say nothing about the GPU)."""
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
p.add_argument("--out", default="profiles", help="directory of the r12_lt_* files")
p.add_argument("--steps", nargs="*", default=["step_time", "learn", "promote"])
p.add_argument("--envs", type=int, nargs="*", default=[65536, 1 << 20], help="batch sizes of step_time")
p.add_argument("--region", type=int, default=64, help="steps per timed region")
p.add_argument("--regions", type=int, default=5)
p.add_argument("--warm", type=int, default=300, help="training steps before the regions")
p.add_argument("--num-envs", type=int, default=65536, help="learn / promote: train.py --num-envs")
p.add_argument("--episodes", type=int, default=40)
p.add_argument("--eval-every", type=int, default=5)
p.add_argument("--limit", type=int, default=420, help="seconds a child process may take")
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

    with open(out("r12_lt_step_time.jsonl"), "w") as fh:
        for B in args.envs:
            learners = {}
            for name, cls in (("rt", pkg.BatchedRowTupleAgent), ("lt", pkg.BatchedLineTupleAgent)):
                agent = cls(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.1, seed=3, device=dev)
                env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                agent.fused_rollout(env, args.warm)                 # trained weights, mid-game boards
                play_env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                play_env.load_state_dict(env.state_dict())
                learners[name] = (agent, env, play_env)
            cases = {f"{n}_{k}": [] for k in ("fused", "play") for n in ("rt", "lt")}
            for name, (agent, env, play_env) in learners.items():   # one untimed region each: first-launch costs
                agent.fused_rollout(env, args.region)
                agent.play_rollout(play_env, args.region)
            for r in range(args.regions):                           # alternating, the order turned round every region
                order = ("rt", "lt") if r % 2 == 0 else ("lt", "rt")
                for name in order:
                    agent, env, _ = learners[name]
                    cases[f"{name}_fused"].append(timed(lambda: agent.fused_rollout(env, args.region)))
                for name in order:
                    agent, _, play_env = learners[name]
                    w = agent.weights.clone()
                    cases[f"{name}_play"].append(timed(lambda: agent.play_rollout(play_env, args.region)))
                    assert torch.equal(w.view(torch.int32), agent.weights.view(torch.int32))
            us = {k: statistics.median(v) * 1e3 / args.region for k, v in cases.items()}
            line = {"case": "lt_step_time", "device": str(dev), "envs": B, "steps_per_region": args.region,
                    "regions": args.regions, "warm_steps": args.warm,
                    **{f"{k}_ms": [round(x, 3) for x in v] for k, v in cases.items()},
                    **{f"{k}_us_per_step": round(v, 3) for k, v in us.items()},
                    "lt_over_rt_fused": round(us["lt_fused"] / us["rt_fused"], 3),
                    "lt_over_rt_play": round(us["lt_play"] / us["rt_play"], 3),
                    "lt_fused_env_steps_per_s": round(B / us["lt_fused"] * 1e6, 1),
                    "lt_play_env_steps_per_s": round(B / us["lt_play"] * 1e6, 1),
                    "lt_train_episodes": learners["lt"][0].stats()["episodes"],
                    "lt_play_valid_move_frac": round(learners["lt"][0].play_stats()["valid_moves"] /
                                                     max(learners["lt"][0].play_stats()["steps"], 1), 6)}
            fh.write(json.dumps(line) + "\n")
            fh.flush()
            print(json.dumps(line), flush=True)


def script(name, *a, log=None):
    cmd = [sys.executable, os.path.join(REPO, name), "--device", args.device.split(":")[0], *a]
    print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO)
    if log:
        with open(log, "w") as fh:
            fh.write(r.stdout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(r.returncode)
    return r.stdout


def train(agent, tag, *a):
    n, e = str(args.num_envs), args.episodes
    script("train.py", "--agent", agent, "--num-envs", n, "--eval-every", str(args.eval_every), "--eval-log",
           out(f"{tag}_eval.jsonl"), "--log", out(f"{tag}.csv"), *a, log=out(f"{tag}.log"))


def evaluate(model, name):
    text = script("evaluate.py", "--model", model, "--num-envs", str(args.num_envs), "--episodes", "2", "--fused")
    with open(out(name), "a") as fh:
        fh.write(text.strip().splitlines()[-1] + "\n")


def learn():
    n, e = args.num_envs, args.episodes
    model = os.path.join(args.models, f"lt_{n}x{e}.pt")
    train("line-tuple", f"r12_lt_train_{n}x{e}", "--episodes", str(e), "--save", model)
    open(out(f"r12_lt_evaluate_{n}x{e}.jsonl"), "w").close()
    evaluate(model, f"r12_lt_evaluate_{n}x{e}.jsonl")


def promote():
    n, e = args.num_envs, args.episodes
    rt, lt = os.path.join(args.models, f"rt_{n}x{e}.pt"), os.path.join(args.models, f"lt_promoted_{n}x{2 * e}.pt")
    train("row-tuple", f"r12_rt_train_{n}x{e}", "--episodes", str(e), "--save", rt)
    train("line-tuple", f"r12_lt_promoted_{n}x{2 * e}", "--episodes", str(2 * e), "--resume", rt, "--save", lt)
    open(out("r12_lt_promoted_evaluate.jsonl"), "w").close()
    evaluate(rt, "r12_lt_promoted_evaluate.jsonl")
    evaluate(lt, "r12_lt_promoted_evaluate.jsonl")


if args.child:
    {"step_time": step_time, "learn": learn, "promote": promote}[args.child]()
    raise SystemExit(0)

os.makedirs(args.out, exist_ok=True)
os.makedirs(os.path.join(REPO, args.models), exist_ok=True)
for step in args.steps:
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", step] + sys.argv[1:]
    t0 = time.time()
    rc = subprocess.run(cmd).returncode
    print(f"[{step}] exit {rc} after {time.time() - t0:.1f} s", flush=True)
    if rc != 0:                                      # a fault, an abort or a time limit: nothing more is started
        raise SystemExit(rc)
