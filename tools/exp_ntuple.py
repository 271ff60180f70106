#!/usr/bin/env python3
"""The 6-tuple afterstate network (four 6-cell patterns on the eight images of the board, 256 MiB) measured beside the
afterstate value learner on the line features (2 MiB), on one build.  Every step that uses the GPU is a child process
under its own `timeout`; the steps are chained, and the first one that fails ends the run.

  step_time   q2048_nt_fused_rollout / q2048_nt_play_rollout and, in the same process, q2048_av_fused_rollout /
              q2048_av_play_rollout at 65,536 and 1,048,576 boards: both learners train --warm steps at that size
              first (trained weights, mid-game boards), then five alternating 64-step regions each by HIP events;
              the median per step and the ratio nt / av                      -> r14_nt_step_time.jsonl
  learn       `train.py --agent ntuple --num-envs 65536 --episodes 40 --eval-every 5 --seed 0` (the command behind
              r13_av_train_65536x40_eval.jsonl, with the other agent) and `evaluate.py --fused` on the saved file
                                                     -> r14_nt_train_65536x40{.log,.csv,_eval.jsonl}, r14_nt_evaluate_65536x40.jsonl
              (another --episodes changes the names accordingly: --episodes 160 is the longer run)
    python tools/exp_ntuple.py --out profiles
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
p.add_argument("--out", default="profiles", help="directory of the r14_nt_* files")
p.add_argument("--steps", nargs="*", default=["step_time", "learn"])
p.add_argument("--envs", type=int, nargs="*", default=[65536, 1 << 20], help="batch sizes of step_time")
p.add_argument("--region", type=int, default=64, help="steps per timed region")
p.add_argument("--regions", type=int, default=5)
p.add_argument("--warm", type=int, default=300, help="training steps before the regions")
p.add_argument("--num-envs", type=int, default=65536, help="learn: train.py --num-envs")
p.add_argument("--episodes", type=int, default=40)
p.add_argument("--eval-every", type=int, default=5)
p.add_argument("--seed", type=int, default=0, help="learn: train.py --seed")
p.add_argument("--limit", type=int, default=420, help="seconds a child process may take")
p.add_argument("--child", default="", help="(internal) the step this process runs itself")
p.add_argument("--models", default="models", help="where the saved learner goes (relative to the repository)")
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

    with open(out("r14_nt_step_time.jsonl"), "w") as fh:
        for B in args.envs:
            learners = {}
            for name, cls in (("av", pkg.BatchedAfterstateAgent), ("nt", pkg.BatchedNTupleAgent)):
                agent = cls(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.1, seed=3, device=dev)
                env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                agent.fused_rollout(env, args.warm)                 # trained weights, mid-game boards
                play_env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
                play_env.load_state_dict(env.state_dict())
                learners[name] = (agent, env, play_env)
            cases = {f"{n}_{k}": [] for k in ("fused", "play") for n in ("av", "nt")}
            for name, (agent, env, play_env) in learners.items():   # one untimed region each: first-launch costs
                agent.fused_rollout(env, args.region)
                agent.play_rollout(play_env, args.region)
            for r in range(args.regions):                           # alternating, the order turned round every region
                order = ("av", "nt") if r % 2 == 0 else ("nt", "av")
                for name in order:
                    agent, env, _ = learners[name]
                    cases[f"{name}_fused"].append(timed(lambda: agent.fused_rollout(env, args.region)))
                for name in order:
                    agent, _, play_env = learners[name]
                    # The snapshot goes through the host.  A device-to-device `clone()` of the 256 MiB issued after a
                    # learning launch of 65,536 racing lanes came back with the older value in 75 of 1.5 million
                    # touched entries, while every later read of the weights -- kernels, a second clone, a host
                    # copy -- agreed with each other; the host copy is what the tests and checkpoints read.
                    w = agent.weights.cpu()
                    cases[f"{name}_play"].append(timed(lambda: agent.play_rollout(play_env, args.region)))
                    assert torch.equal(w.view(torch.int32), agent.weights.cpu().view(torch.int32)), f"{name}: the player wrote"
                    del w
            us = {k: statistics.median(v) * 1e3 / args.region for k, v in cases.items()}
            nt = learners["nt"][0]
            line = {"case": "nt_step_time", "device": str(dev), "envs": B, "steps_per_region": args.region,
                    "regions": args.regions, "warm_steps": args.warm,
                    **{f"{k}_ms": [round(x, 3) for x in v] for k, v in cases.items()},
                    **{f"{k}_us_per_step": round(v, 3) for k, v in us.items()},
                    "nt_over_av_fused": round(us["nt_fused"] / us["av_fused"], 3),
                    "nt_over_av_play": round(us["nt_play"] / us["av_play"], 3),
                    "nt_fused_env_steps_per_s": round(B / us["nt_fused"] * 1e6, 1),
                    "nt_play_env_steps_per_s": round(B / us["nt_play"] * 1e6, 1),
                    "nt_train_episodes": nt.stats()["episodes"],
                    "nt_weights_touched": int(torch.count_nonzero(nt.weights).item()),
                    "nt_play_valid_move_frac": round(nt.play_stats()["valid_moves"] / max(nt.play_stats()["steps"], 1), 6)}
            fh.write(json.dumps(line) + "\n")
            fh.flush()
            print(json.dumps(line), flush=True)


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


def learn():
    n, e = args.num_envs, args.episodes
    tag, model = f"r14_nt_train_{n}x{e}", os.path.join(args.models, f"nt_{n}x{e}.pt")
    script("train.py", "--agent", "ntuple", "--num-envs", str(n), "--episodes", str(e), "--seed", str(args.seed),
           "--eval-every", str(args.eval_every), "--eval-log", out(f"{tag}_eval.jsonl"), "--log", out(f"{tag}.csv"),
           "--save", model, log=out(f"{tag}.log"))
    text = script("evaluate.py", "--model", model, "--num-envs", str(n), "--episodes", "2", "--fused")
    with open(out(f"r14_nt_evaluate_{n}x{e}.jsonl"), "w") as fh:
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
