#!/usr/bin/env python3
"""Symmetry folding (Q2048_FLAG_SYMMETRIC) against the plain table, in one process, timed by HIP events.

Two learners on the same seed -- `BatchedQLearningAgent(symmetric=False / True)`, 4x4, a SHARED table of 2^30 slots
(32 GiB) that cannot grow and closes its key set at freeze_load 0.5, epsilon 0.95 -- and 1 Mi envs each:
  step_time   5 warm-up steps, then alternating pairs of 20-step launches (plain first, then folded first, ...), five
              of each; the median per step, and the difference              -> {"case": "step_time"}
  rows        both runs go on in 20-step launches until their key set closes (or --max-steps); the kernels' insert
              counter is read every --every steps                            -> {"case": "rows"} per reading
  summary     rows per env-step over the first 2e9 env-steps (or up to the freeze, whichever comes first) and the
              env-steps at which freeze_load was reached, both ways          -> {"case": "summary"}
    python tools/exp_symmetric.py > profiles/r09_symmetric.jsonl
`--device cpu --envs 2048 --cap-log2 16 --max-steps 400` rehearses the script on the CPU twin (host clock; its times
say nothing about the GPU)."""
import argparse
import importlib
import json
import os
import sys
import time
import warnings

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("2048_q-learning_amd")

p = argparse.ArgumentParser()
p.add_argument("--device", default="cuda:0")
p.add_argument("--envs", type=int, default=1 << 20)
p.add_argument("--cap-log2", type=int, default=30)
p.add_argument("--launch", type=int, default=20, help="steps per launch (the bench's launch shape)")
p.add_argument("--warmup", type=int, default=5)
p.add_argument("--pairs", type=int, default=5)
p.add_argument("--every", type=int, default=200, help="steps between readings of the insert counter")
p.add_argument("--max-steps", type=int, default=40000)
p.add_argument("--first", type=float, default=2e9, help="env-steps of the rows-per-env-step figure")
args = p.parse_args()
dev = torch.device(args.device)
on_gpu = dev.type == "cuda"
if on_gpu:
    torch.cuda.set_device(dev)
warnings.simplefilter("ignore")          # (the freeze warning is what the run waits for)


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


def median(xs):
    return sorted(xs)[len(xs) // 2]


def learner(symmetric):
    env = pkg.BatchedGame2048Env(args.envs, 4, dev, seed=9, env_id0=0)
    agent = pkg.BatchedQLearningAgent(1000, learning_rate=0.1, discount_factor=0.99, exploration_rate=0.95,
                                      capacity_log2=args.cap_log2, seed=9, env_id0=0, device=dev,
                                      placement="auto" if on_gpu else "plain", freeze_load=0.5, symmetric=symmetric)
    return env, agent


runs = {"plain": learner(False), "symmetric": learner(True)}
B, K = args.envs, args.launch
for env, agent in runs.values():
    agent.fused_rollout(env, args.warmup)
times = {k: [] for k in runs}
for r in range(args.pairs):
    for name in (("plain", "symmetric") if r % 2 == 0 else ("symmetric", "plain")):
        env, agent = runs[name]
        times[name].append(timed(lambda: agent.fused_rollout(env, K)))
us = {k: round(median(v) * 1e3 / K, 3) for k, v in times.items()}
print(json.dumps({"case": "step_time", "device": str(dev), "envs": B, "cap_log2": args.cap_log2, "steps_per_launch": K,
                  "warmup_steps": args.warmup, "pairs": args.pairs,
                  "plain_ms": [round(t, 3) for t in times["plain"]], "symmetric_ms": [round(t, 3) for t in times["symmetric"]],
                  "plain_us_per_step": us["plain"], "symmetric_us_per_step": us["symmetric"],
                  "symmetric_minus_plain_us": round(us["symmetric"] - us["plain"], 3),
                  "estimate_before_measuring_us": 4.0,
                  "placement": {k: v[1].placement.get("mode") for k, v in runs.items()}}), flush=True)

summary = {}
for name, (env, agent) in runs.items():
    first_rows, first_steps, frozen_at = None, None, None
    while env.ctr < args.max_steps and not agent.frozen:
        for _ in range(max(1, args.every // K)):
            agent.fused_rollout(env, K)
            if agent.frozen:
                break
        st = agent.stats()
        env_steps = env.ctr * B
        print(json.dumps({"case": "rows", "table": name, "steps": env.ctr, "env_steps": env_steps, "rows": st["inserts"],
                          "load": round(st["inserts"] / float(1 << args.cap_log2), 5), "drops": st["drops"],
                          "frozen": agent.frozen}), flush=True)
        if first_rows is None and (env_steps >= args.first or agent.frozen):
            first_rows, first_steps = st["inserts"], env_steps
    if first_rows is None:
        st = agent.stats()
        first_rows, first_steps = st["inserts"], env.ctr * B
    if agent.frozen:
        frozen_at = {"env_steps": agent.frozen_at["at_step"] * B, "rows": agent.frozen_at["rows"]}
    check = agent.verify_table()
    summary[name] = {"rows": first_rows, "env_steps": first_steps, "rows_per_env_step": round(first_rows / first_steps, 5),
                     "frozen_at": frozen_at, "rows_at_end": check["rows"], "steps_at_end": env.ctr,
                     "status": int(agent.status.item())}
out = {"case": "summary", "envs": B, "cap_log2": args.cap_log2, "freeze_load": 0.5, **summary}
a, b = summary["plain"], summary["symmetric"]
out["rows_per_env_step_ratio"] = round(a["rows_per_env_step"] / max(b["rows_per_env_step"], 1e-12), 3)
if a["frozen_at"] and b["frozen_at"]:
    out["env_steps_to_freeze_ratio"] = round(b["frozen_at"]["env_steps"] / a["frozen_at"]["env_steps"], 3)
print(json.dumps(out), flush=True)
