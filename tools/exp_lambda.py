#!/usr/bin/env python3
"""TD(lambda) with a truncated trace for the 6-tuple afterstate network (q2048_nt_lambda_*) measured beside the plain
learner (q2048_nt_*) of the same build.  Every step that uses the GPU is a child process under its own `timeout`; the
steps are chained, and the first one that fails ends the run.

  step_time   q2048_nt_lambda_fused_rollout at h = 1 and h = 3 (lambda 0.5) and, in the same process,
              q2048_nt_fused_rollout at 65,536 and 1,048,576 boards: every learner trains --warm steps at that size first
              (trained weights, mid-game boards), then five alternating 64-step regions each by HIP events; the median
              per step, the ratio to the plain step, the mean trace length n of the lanes after the last region (what the
              next step starts from, before its cut) and what the count of requests predicts from it,
              (320 + 64 n) / 320                                                     -> r21_lambda_step_time.jsonl
  learn       one child per value of --episodes: `train.py --agent ntuple --trace-lambda 0.5 --num-envs 65536
              --episodes E --eval-every 5 --seed 0` (the command behind r14_nt_train_65536x{40,160}_eval.jsonl with the
              flag), then `evaluate.py --fused` and `--fused --search` on the saved file
                                    -> r21_lambda_train_65536x{E}{.log,.csv,_eval.jsonl}, r21_lambda_evaluate_65536x{E}.jsonl
    python tools/exp_lambda.py --out profiles
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
p.add_argument("--out", default="profiles", help="directory of the r21_lambda_* files")
p.add_argument("--steps", nargs="*", default=["step_time", "learn"])
p.add_argument("--envs", type=int, nargs="*", default=[65536, 1 << 20], help="batch sizes of step_time")
p.add_argument("--region", type=int, default=64, help="steps per timed region")
p.add_argument("--regions", type=int, default=5)
p.add_argument("--warm", type=int, default=300, help="training steps before the regions")
p.add_argument("--trace-lambda", default="0.5", help="lambda of both steps, as written")
p.add_argument("--num-envs", type=int, default=65536, help="learn: train.py --num-envs")
p.add_argument("--episodes", nargs="*", default=["40", "160"], help="learn: one run per value")
p.add_argument("--eval-every", type=int, default=5)
p.add_argument("--seed", type=int, default=0, help="learn: train.py --seed")
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
    lam = float(args.trace_lambda)

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

    names = ("nt", "lambda_h1", "lambda_h3")
    with open(out("r21_lambda_step_time.jsonl"), "w") as fh:
        for B in args.envs:
            learners = {}
            for name, kw in zip(names, ({}, {"trace_lambda": lam, "trace_depth": 1}, {"trace_lambda": lam, "trace_depth": 3})):
                agent = pkg.BatchedNTupleAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.1, seed=3,
                                               device=dev, **kw)
                env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                agent.fused_rollout(env, args.warm)                 # trained weights, mid-game boards
                learners[name] = (agent, env)
            cases = {f"{name}_fused": [] for name in names}
            for agent, env in learners.values():                    # one untimed region each: first-launch costs
                agent.fused_rollout(env, args.region)
            for r in range(args.regions):                           # alternating, the order turned round every region
                for name in (names if r % 2 == 0 else names[::-1]):
                    agent, env = learners[name]
                    cases[f"{name}_fused"].append(timed(lambda: agent.fused_rollout(env, args.region)))
            us = {k: statistics.median(v) * 1e3 / args.region for k, v in cases.items()}
            line = {"case": "lambda_step_time", "device": str(dev), "envs": B, "steps_per_region": args.region,
                    "regions": args.regions, "warm_steps": args.warm, "lambda": lam,
                    **{f"{k}_ms": [round(x, 3) for x in v] for k, v in cases.items()},
                    **{f"{k}_us_per_step": round(v, 3) for k, v in us.items()},
                    "nt_fused_env_steps_per_s": round(B / us["nt_fused"] * 1e6, 1)}
            for name in names[1:]:
                agent = learners[name][0]
                n_mean = float(agent.trace[:, 0].to(torch.float64).mean().item())
                line.update({f"{name}_over_nt_fused": round(us[f"{name}_fused"] / us["nt_fused"], 3),
                             f"{name}_mean_trace_length": round(n_mean, 4),
                             f"{name}_requests_predict": round((320 + 64 * n_mean) / 320, 3),
                             f"{name}_fused_env_steps_per_s": round(B / us[f"{name}_fused"] * 1e6, 1),
                             f"{name}_train_episodes": agent.stats()["episodes"]})
            line["nt_train_episodes"] = learners["nt"][0].stats()["episodes"]
            fh.write(json.dumps(line) + "\n")
            fh.flush()
            print(json.dumps(line), flush=True)
            del learners, agent


def script(name, *a, log=None):
    cmd = [sys.executable, os.path.join(REPO, name), "--device", args.device.split(":")[0], *a]
    print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=args.limit)
    if log:
        with open(log, "w") as fh:
            fh.write(r.stdout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(r.returncode)
    return r.stdout


def learn(episodes):
    n = args.num_envs
    tag, model = f"r21_lambda_train_{n}x{episodes}", os.path.join(args.models, f"lambda_{n}x{episodes}.pt")
    script("train.py", "--agent", "ntuple", "--trace-lambda", args.trace_lambda, "--num-envs", str(n), "--episodes", episodes,
           "--seed", str(args.seed), "--eval-every", str(args.eval_every), "--eval-log", out(f"{tag}_eval.jsonl"),
           "--log", out(f"{tag}.csv"), "--save", model, log=out(f"{tag}.log"))
    with open(out(f"r21_lambda_evaluate_{n}x{episodes}.jsonl"), "w") as fh:
        for search in ((), ("--search",)):
            text = script("evaluate.py", "--model", model, "--num-envs", str(n), "--episodes", "2", "--fused", *search)
            line = json.loads(text.strip().splitlines()[-1])
            fh.write(json.dumps({"case": "lambda_strength", "lambda": float(args.trace_lambda), "episodes": int(episodes),
                                 "search": int(bool(search)), **line}) + "\n")
            fh.flush()
    os.remove(os.path.join(REPO, model))             # 256 MiB a run: the profiles are what is kept


if args.child:
    what, *cell = args.child.split(":")
    {"step_time": step_time, "learn": learn}[what](*cell)
    raise SystemExit(0)

os.makedirs(args.out, exist_ok=True)
os.makedirs(os.path.join(REPO, args.models), exist_ok=True)
children = []
for step in args.steps:
    children += [step] if step != "learn" else [f"learn:{e}" for e in args.episodes]
for child in children:
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", child] + sys.argv[1:]
    t0 = time.time()
    rc = subprocess.run(cmd).returncode
    print(f"[{child}] exit {rc} after {time.time() - t0:.1f} s", flush=True)
    if rc != 0:                                      # a fault, an abort or a time limit: nothing more is started
        raise SystemExit(rc)
