#!/usr/bin/env python3
"""The synchronous batch step of the 6-tuple afterstate network (q2048_nt_sync_*) measured beside the plain learner
(q2048_nt_*) of the same build.  Every step that uses the GPU is a child process under its own `timeout`; the steps are
chained, and the first one that fails ends the run.

  step_time   q2048_nt_sync_fused_rollout and, in the same process, q2048_nt_fused_rollout at 65,536 and 1,048,576
              boards: both learners train --warm steps at that size first (epsilon 0.1: trained weights, mid-game
              boards), then five alternating 64-step regions each by HIP events; the median per step and the ratio to the
              plain step of the same run                                            -> r22_sync_step_time.jsonl
  split       the same synchronous steps once more under `rocprofv3 --kernel-trace` (a process of its own): the mean
              duration of k_nt_sync_step (phase A) and of k_nt_sync_apply (phase B) over the launches after the warm-up
              and the untimed region, per size; the lines are appended to r22_sync_step_time.jsonl
  learn       one child per value of --episodes: `train.py --agent ntuple --synchronous --num-envs 65536 --episodes E
              --eval-every 5 --seed 0` (the command behind r14_nt_train_65536x{40,160}_eval.jsonl with the flag), then
              `evaluate.py --fused` and `--fused --search` on the saved file
                                    -> r22_sync_train_65536x{E}{.log,.csv,_eval.jsonl}, r22_sync_evaluate_65536x{E}.jsonl
  repeat      the first --episodes command a second time: the two eval logs and the two saved files are compared byte
              for byte (the weights as float32 bit patterns too)                   -> r22_sync_repeat.jsonl
    python tools/exp_sync.py --out profiles
`--device cpu --envs 2048 --num-envs 256 --episodes 4 --eval-every 2 --steps step_time learn repeat` rehearses the script
on the CPU twin (host clock; its times say nothing about the GPU)."""
import argparse
import csv
import glob
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

p = argparse.ArgumentParser()
p.add_argument("--device", default="cuda:0")
p.add_argument("--out", default="profiles", help="directory of the r22_sync_* files")
p.add_argument("--steps", nargs="*", default=["step_time", "split", "learn", "repeat"])
p.add_argument("--envs", type=int, nargs="*", default=[65536, 1 << 20], help="batch sizes of step_time")
p.add_argument("--region", type=int, default=64, help="steps per timed region")
p.add_argument("--regions", type=int, default=5)
p.add_argument("--warm", type=int, default=300, help="training steps before the regions")
p.add_argument("--num-envs", type=int, default=65536, help="learn: train.py --num-envs")
p.add_argument("--episodes", nargs="*", default=["40", "160"], help="learn: one run per value")
p.add_argument("--eval-every", type=int, default=5)
p.add_argument("--seed", type=int, default=0, help="learn: train.py --seed")
p.add_argument("--limit", type=int, default=420, help="seconds a child process may take")
p.add_argument("--child", default="", help="(internal) the step this process runs itself")
p.add_argument("--models", default="models", help="where the saved learners go (relative to the repository)")
args = p.parse_args()
out = lambda name: os.path.join(os.path.abspath(args.out), name)  # noqa: E731
NAMES = ("nt", "sync")


def learners_at(pkg, dev, B):
    out_ = {}
    for name, kw in zip(NAMES, ({}, {"synchronous": True})):
        agent = pkg.BatchedNTupleAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.1, seed=3,
                                       device=dev, **kw)
        env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
        agent.fused_rollout(env, args.warm)                 # trained weights, mid-game boards
        out_[name] = (agent, env)
    return out_


def setup():
    import importlib

    import torch

    sys.path.insert(0, REPO)
    pkg = importlib.import_module("2048_q-learning_amd")
    dev = torch.device(args.device)
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    return pkg, torch, dev


def step_time():
    pkg, torch, dev = setup()
    on_gpu = dev.type == "cuda"

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

    with open(out("r22_sync_step_time.jsonl"), "w") as fh:
        for B in args.envs:
            learners = learners_at(pkg, dev, B)
            cases = {f"{name}_fused": [] for name in NAMES}
            for agent, env in learners.values():                    # one untimed region each: first-launch costs
                agent.fused_rollout(env, args.region)
            for r in range(args.regions):                           # alternating, the order turned round every region
                for name in (NAMES if r % 2 == 0 else NAMES[::-1]):
                    agent, env = learners[name]
                    cases[f"{name}_fused"].append(timed(lambda: agent.fused_rollout(env, args.region)))
            us = {k: statistics.median(v) * 1e3 / args.region for k, v in cases.items()}
            line = {"case": "sync_step_time", "device": str(dev), "envs": B, "steps_per_region": args.region,
                    "regions": args.regions, "warm_steps": args.warm,
                    **{f"{k}_ms": [round(x, 3) for x in v] for k, v in cases.items()},
                    **{f"{k}_us_per_step": round(v, 3) for k, v in us.items()},
                    "sync_over_nt_fused": round(us["sync_fused"] / us["nt_fused"], 3),
                    **{f"{name}_fused_env_steps_per_s": round(B / us[f"{name}_fused"] * 1e6, 1) for name in NAMES},
                    **{f"{name}_train_episodes": learners[name][0].stats()["episodes"] for name in NAMES}}
            fh.write(json.dumps(line) + "\n")
            fh.flush()
            print(json.dumps(line), flush=True)
            del learners, agent, env


def split_body():
    """what runs under the profiler: per size, the warm-up and then --regions regions of the synchronous learner alone"""
    pkg, torch, dev = setup()
    for B in args.envs:
        agent = pkg.BatchedNTupleAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.1, seed=3,
                                       device=dev, synchronous=True)
        env = pkg.BatchedGame2048Env(B, 4, dev, 3, 0)
        agent.fused_rollout(env, args.warm + args.region * (1 + args.regions))
        torch.cuda.synchronize()
        del agent, env


def split():
    """Kernel durations by grid size (one block per 256 boards tells the sizes apart) out of the kernel trace."""
    work = out("r22_sync_split_trace")
    shutil.rmtree(work, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", work, "-o", "split", "--", sys.executable,
           os.path.abspath(__file__)] + passed_on() + ["--child", "split_body"]
    subprocess.run(cmd, check=True, timeout=args.limit)
    found = glob.glob(os.path.join(work, "**", "*kernel_trace.csv"), recursive=True)
    if not found:
        raise SystemExit(f"no kernel trace under {work}")
    total = {}
    with open(found[0]) as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            for short in ("k_nt_sync_step", "k_nt_sync_apply"):
                if short in name:
                    key = (int(row["Grid_Size"] if "Grid_Size" in row else row["Grid_Size_X"]), short)
                    total.setdefault(key, []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    shutil.rmtree(work, ignore_errors=True)
    with open(out("r22_sync_step_time.jsonl"), "a") as fh:
        for grid in sorted({g for g, _ in total}):
            last = args.region * args.regions                 # in launch order: what step_time's regions ran
            (a_ns, a_n), (b_ns, b_n) = ((sum(e - b for b, e in sorted(total[(grid, k)])[-last:]), len(total[(grid, k)][-last:]))
                                        for k in ("k_nt_sync_step", "k_nt_sync_apply"))
            line = {"case": "sync_phase_split", "source": "rocprofv3 --kernel-trace, a run of its own, its last launches",
                    "grid_threads": grid, "launches_each": a_n, "phase_a_us_per_step": round(a_ns / a_n / 1e3, 3),
                    "phase_b_us_per_step": round(b_ns / b_n / 1e3, 3),
                    "phase_a_share": round(a_ns / (a_ns + b_ns), 4), "phase_b_share": round(b_ns / (a_ns + b_ns), 4)}
            assert a_n == b_n
            fh.write(json.dumps(line) + "\n")
            print(json.dumps(line), flush=True)


def passed_on():
    """this process's arguments without --child"""
    argv = sys.argv[1:]
    while "--child" in argv:
        k = argv.index("--child")
        del argv[k:k + 2]
    return argv


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


def train(episodes, tag, model):
    n = args.num_envs
    script("train.py", "--agent", "ntuple", "--synchronous", "--num-envs", str(n), "--episodes", episodes,
           "--seed", str(args.seed), "--eval-every", str(args.eval_every), "--eval-log", out(f"{tag}_eval.jsonl"),
           "--log", out(f"{tag}.csv"), "--save", model, log=out(f"{tag}.log"))


def model_of(episodes, suffix=""):
    return os.path.join(args.models, f"sync_{args.num_envs}x{episodes}{suffix}.pt")


def learn(episodes):
    n = args.num_envs
    model = model_of(episodes)
    train(episodes, f"r22_sync_train_{n}x{episodes}", model)
    with open(out(f"r22_sync_evaluate_{n}x{episodes}.jsonl"), "w") as fh:
        for search in ((), ("--search",)):
            text = script("evaluate.py", "--model", model, "--num-envs", str(n), "--episodes", "2", "--fused", *search)
            line = json.loads(text.strip().splitlines()[-1])
            fh.write(json.dumps({"case": "sync_strength", "episodes": int(episodes), "search": int(bool(search)), **line}) + "\n")
            fh.flush()
    if episodes != args.episodes[0]:                 # the first is kept for `repeat`; 256 MiB a run: the profiles are what is kept
        os.remove(os.path.join(REPO, model))


def repeat():
    """The first learning command again, from nothing: the eval log and the saved weights must be the first run's."""
    import torch

    n, episodes = args.num_envs, args.episodes[0]
    first, again = model_of(episodes), model_of(episodes, "_again")
    tag = f"r22_sync_repeat_{n}x{episodes}"
    train(episodes, tag, again)
    digest = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()      # noqa: E731
    logs = [out(f"r22_sync_train_{n}x{episodes}_eval.jsonl"), out(f"{tag}_eval.jsonl")]
    a, b = (torch.load(os.path.join(REPO, m), map_location="cpu", weights_only=False) for m in (first, again))
    wa, wb = a["weights"].view(torch.int32), b["weights"].view(torch.int32)
    line = {"case": "sync_repeat", "command": f"train.py --agent ntuple --synchronous --num-envs {n} --episodes {episodes} "
                                              f"--eval-every {args.eval_every} --seed {args.seed}",
            "device": args.device, "eval_logs_identical": digest(logs[0]) == digest(logs[1]),
            "eval_log_sha256": [digest(x) for x in logs],
            "weights_identical": bool(torch.equal(wa, wb)), "weights_differing": int((wa != wb).sum()),
            "weights_nonzero": int((wa != 0).sum()),
            "boards_identical": bool(torch.equal(a["env"]["boards"], b["env"]["boards"])),
            "stats_i_identical": bool(torch.equal(a["stats_i"], b["stats_i"])),
            "weights_sha256": [hashlib.sha256(w.numpy().tobytes()).hexdigest() for w in (wa, wb)]}
    with open(out("r22_sync_repeat.jsonl"), "w") as fh:
        fh.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)
    for name in (f"{tag}_eval.jsonl", f"{tag}.csv", f"{tag}.log"):
        os.remove(out(name))
    for m in (first, again):
        os.remove(os.path.join(REPO, m))
    if not (line["eval_logs_identical"] and line["weights_identical"]):
        raise SystemExit("the repeat differs")


if args.child:
    what, *cell = args.child.split(":")
    {"step_time": step_time, "split": split, "split_body": split_body, "learn": learn, "repeat": repeat}[what](*cell)
    raise SystemExit(0)

os.makedirs(args.out, exist_ok=True)
os.makedirs(os.path.join(REPO, args.models), exist_ok=True)
children = []
for step in args.steps:
    children += [step] if step != "learn" else [f"learn:{e}" for e in args.episodes]
for child in children:
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__)] + sys.argv[1:] + ["--child", child]
    t0 = time.time()
    rc = subprocess.run(cmd).returncode
    print(f"[{child}] exit {rc} after {time.time() - t0:.1f} s", flush=True)
    if rc != 0:                                      # a fault, an abort or a time limit: nothing more is started
        raise SystemExit(rc)
