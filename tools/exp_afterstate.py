#!/usr/bin/env python3
"""The afterstate value learner (one value per line entry, 2 MiB; a state judged by its four moved boards) measured
beside the line-tuple learner (a Q value per line entry and action, 8 MiB), on one build.  Every step that uses the GPU
is a child process under its own `timeout`; the steps are chained, and the first one that fails ends the run.

  step_time   q2048_av_fused_rollout / q2048_av_play_rollout and, in the same process, q2048_lt_fused_rollout /
              q2048_lt_play_rollout at 65,536 and 1,048,576 boards: both learners train --warm steps at that size
              first (trained weights, mid-game boards), then five alternating 64-step regions each by HIP events;
              the median per step and the ratio av / lt                      -> r13_av_step_time.jsonl
  learn       `train.py --agent afterstate --num-envs 65536 --episodes 40 --eval-every 5` (the command behind
              r12_lt_train_65536x40_eval.jsonl, with the other agent), once per value of --alphas, and
              `evaluate.py --fused` on each saved file
                                                     -> r13_av_train_65536x40{.log,.csv,_eval.jsonl}, r13_av_evaluate_65536x40.jsonl
                                                        (a value of --alphas other than 0.1 adds _alphaX to the names)
    python tools/exp_afterstate.py --out profiles
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
p.add_argument("--out", default="profiles", help="directory of the r13_av_* files")
p.add_argument("--steps", nargs="*", default=["step_time", "learn"])
p.add_argument("--envs", type=int, nargs="*", default=[65536, 1 << 20], help="batch sizes of step_time")
p.add_argument("--region", type=int, default=64, help="steps per timed region")
p.add_argument("--regions", type=int, default=5)
p.add_argument("--warm", type=int, default=300, help="training steps before the regions")
p.add_argument("--num-envs", type=int, default=65536, help="learn: train.py --num-envs")
p.add_argument("--episodes", type=int, default=40)
p.add_argument("--eval-every", type=int, default=5)
p.add_argument("--alphas", type=float, nargs="*", default=[0.1], help="learn: one training run per learning rate")
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

    with open(out("r13_av_step_time.jsonl"), "w") as fh:
        for B in args.envs:
            learners = {}
            for name, cls in (("lt", pkg.BatchedLineTupleAgent), ("av", pkg.BatchedAfterstateAgent)):
                agent = cls(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.1, seed=3, device=dev)
                env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                agent.fused_rollout(env, args.warm)                 # trained weights, mid-game boards
                play_env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                play_env.load_state_dict(env.state_dict())
                learners[name] = (agent, env, play_env)
            cases = {f"{n}_{k}": [] for k in ("fused", "play") for n in ("lt", "av")}
            for name, (agent, env, play_env) in learners.items():   # one untimed region each: first-launch costs
                agent.fused_rollout(env, args.region)
                agent.play_rollout(play_env, args.region)
            for r in range(args.regions):                           # alternating, the order turned round every region
                order = ("lt", "av") if r % 2 == 0 else ("av", "lt")
                for name in order:
                    agent, env, _ = learners[name]
                    cases[f"{name}_fused"].append(timed(lambda: agent.fused_rollout(env, args.region)))
                for name in order:
                    agent, _, play_env = learners[name]
                    w = agent.weights.clone()
                    cases[f"{name}_play"].append(timed(lambda: agent.play_rollout(play_env, args.region)))
                    assert torch.equal(w.view(torch.int32), agent.weights.view(torch.int32))
            us = {k: statistics.median(v) * 1e3 / args.region for k, v in cases.items()}
            av = learners["av"][0]
            line = {"case": "av_step_time", "device": str(dev), "envs": B, "steps_per_region": args.region,
                    "regions": args.regions, "warm_steps": args.warm,
                    **{f"{k}_ms": [round(x, 3) for x in v] for k, v in cases.items()},
                    **{f"{k}_us_per_step": round(v, 3) for k, v in us.items()},
                    "av_over_lt_fused": round(us["av_fused"] / us["lt_fused"], 3),
                    "av_over_lt_play": round(us["av_play"] / us["lt_play"], 3),
                    "av_fused_env_steps_per_s": round(B / us["av_fused"] * 1e6, 1),
                    "av_play_env_steps_per_s": round(B / us["av_play"] * 1e6, 1),
                    "av_train_episodes": av.stats()["episodes"],
                    "av_play_valid_move_frac": round(av.play_stats()["valid_moves"] / max(av.play_stats()["steps"], 1), 6)}
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


def learn():
    n, e = args.num_envs, args.episodes
    for alpha in args.alphas:
        suffix = "" if alpha == 0.1 else f"_alpha{alpha:g}"
        tag, model = f"r13_av_train_{n}x{e}{suffix}", os.path.join(args.models, f"av_{n}x{e}{suffix}.pt")
        script("train.py", "--agent", "afterstate", "--num-envs", str(n), "--episodes", str(e), "--alpha", str(alpha),
               "--eval-every", str(args.eval_every), "--eval-log", out(f"{tag}_eval.jsonl"), "--log", out(f"{tag}.csv"),
               "--save", model, log=out(f"{tag}.log"))
        text = script("evaluate.py", "--model", model, "--num-envs", str(n), "--episodes", "2", "--fused")
        with open(out(f"r13_av_evaluate_{n}x{e}{suffix}.jsonl"), "w") as fh:
            fh.write(text.strip().splitlines()[-1] + "\n")


if args.child:
    {"step_time": step_time, "learn": learn}[args.child]()
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
