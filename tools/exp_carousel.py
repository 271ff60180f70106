#!/usr/bin/env python3
"""Carousel shaping (q2048_car_*) measured beside the staged learner of the same build.  Every step that uses the GPU is
a child process under its own `timeout`; the steps are chained, and the first one that fails ends the run.

  step_time   q2048_car_fused_rollout and q2048_car_commit, called as the agent calls them, and in the same process
              q2048_nts_fused_rollout, with the threshold 2048 (which no board reaches in the warm steps: nothing is
              recorded) and with the thresholds 32 and 128 (records, restarts from the pool and commits in every
              region), at 65,536 and 1,048,576 boards: both learners train --warm steps at that size first (the
              carousel's pool fills on the way), then five alternating 64-step regions each by HIP events -- the
              learner and its commit timed apart; the medians per step, the commit per launch and the ratios
              car / nts.  The yardstick is the staged kernel of the same run
                                                                                    -> r19_carousel_step_time.jsonl
  strength    `train.py --agent ntuple --num-envs 65536 --episodes 40 --eval-every 5 --seed 0` three ways: plain, with
              `--stage-tiles 2048`, and with `--stage-tiles 2048 --carousel 4096`.  train.main runs in the child with
              the agent's fused_rollout wrapped: after every launch the boards are counted by stage on the device, so
              the share of env-steps a stage received is a sample at every launch boundary (every --steps-per-launch
              steps, all lanes), not a count of every step
                        -> r19_carousel_train_{plain,staged,carousel}{.log,_eval.jsonl}, r19_carousel_stage_share.jsonl
    python tools/exp_carousel.py --out profiles
`--device cpu --envs 2048 --num-envs 256 --episodes 4 --eval-every 2 --warm 50 --regions 2 --region 4 --carousel 64
--stage-tiles 64` rehearses the script on the CPU twin (host clock; its times say nothing about the GPU).  One seed: the
strength figures are one run each."""
import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

p = argparse.ArgumentParser()
p.add_argument("--device", default="cuda:0")
p.add_argument("--out", default="profiles", help="directory of the r19_carousel_* files")
p.add_argument("--steps", nargs="*", default=["step_time", "strength"])
p.add_argument("--envs", type=int, nargs="*", default=[65536, 1 << 20], help="batch sizes of step_time")
p.add_argument("--region", type=int, default=64, help="steps per timed region")
p.add_argument("--regions", type=int, default=5)
p.add_argument("--warm", type=int, default=300, help="training steps before the regions")
p.add_argument("--num-envs", type=int, default=65536, help="strength: train.py --num-envs")
p.add_argument("--episodes", type=int, default=40)
p.add_argument("--eval-every", type=int, default=5)
p.add_argument("--stage-tiles", default="2048")
p.add_argument("--step-tiles", nargs="*", default=["2048", "32,128"],
               help="step_time: the thresholds of its cases (no board reaches 2048 in the warm steps: that case records "
                    "nothing; with 32,128 records, restarts from the pool and commits are part of every region)")
p.add_argument("--carousel", type=int, default=4096)
p.add_argument("--seed", type=int, default=0, help="strength: train.py --seed")
p.add_argument("--limit", type=int, default=420, help="seconds a child process may take")
p.add_argument("--child", default="", help="(internal) the step this process runs itself")
p.add_argument("--models", default="models", help="where the saved learners go (relative to the repository)")
args = p.parse_args()
out = lambda name: os.path.join(os.path.abspath(args.out), name)  # noqa: E731
TILES = tuple(int(t) for t in args.stage_tiles.split(","))
RUNS = {"plain": (), "staged": ("--stage-tiles", args.stage_tiles),
        "carousel": ("--stage-tiles", args.stage_tiles, "--carousel", str(args.carousel))}


def package():
    import importlib

    import torch

    sys.path.insert(0, REPO)
    pkg = importlib.import_module("2048_q-learning_amd")
    dev = torch.device(args.device)
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    return pkg, torch, dev


def step_time():
    pkg, torch, dev = package()
    on_gpu = dev.type == "cuda"
    ptr = lambda t: t.data_ptr()      # noqa: E731

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

    def learner(tiles, carousel):
        return pkg.BatchedNTupleAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.1, seed=3, device=dev,
                                      stage_tiles=tiles, carousel=carousel)

    L = pkg._native.lib_for(dev)
    with open(out("r19_carousel_step_time.jsonl"), "w") as fh:
        for tiles, B in ((tuple(int(t) for t in spec.split(",")), B) for spec in args.step_tiles for B in args.envs):
            nts, car = learner(tiles, 0), learner(tiles, args.carousel)
            env_n, env_c = (pkg.BatchedGame2048Env(B, 4, dev, 3, 0) for _ in range(2))
            for _ in range(max(args.warm // args.region, 1)):          # trained weights, mid-game boards, a filled pool
                nts.fused_rollout(env_n, args.region)
                car.fused_rollout(env_c, args.region)

            def car_learn():
                pkg._native.check(L.q2048_car_fused_rollout(
                    ptr(env_c.boards), ptr(env_c.aux), ptr(car.weights), car._stages, ptr(car.carousel_pool),
                    ptr(car.carousel_counts), ptr(car.carousel_fresh), car.carousel, B, args.region, float(car.epsilon),
                    float(car.lr), float(car.gamma), car.seed, car.env_id0, car.ctr & 0xFFFFFFFF, ptr(car.stats_i),
                    ptr(car.stats_f), ptr(car.status), None), "car_fused_rollout")
                car.ctr += args.region
                env_c.ctr += args.region

            def car_commit():
                pkg._native.check(L.q2048_car_commit(ptr(car.carousel_pool), ptr(car.carousel_counts), ptr(car.carousel_fresh),
                                                     car._stages, car.carousel, B, None), "car_commit")

            cases = {"nts_fused": [], "car_fused": [], "car_commit": []}
            counts_before = car.carousel_summary()["counts"]
            for r in range(args.regions):                           # alternating, the order turned round every region
                for name in (("nts", "car") if r % 2 == 0 else ("car", "nts")):
                    if name == "nts":
                        cases["nts_fused"].append(timed(lambda: nts.fused_rollout(env_n, args.region)))
                    else:
                        cases["car_fused"].append(timed(car_learn))
                        cases["car_commit"].append(timed(car_commit))
            med = {k: statistics.median(v) for k, v in cases.items()}
            counts = car.carousel_summary()["counts"]
            line = {"case": "carousel_step_time", "device": str(dev), "envs": B, "steps_per_region": args.region,
                    "regions": args.regions, "warm_steps": args.warm, "stage_tiles": list(tiles), "carousel": args.carousel,
                    **{f"{k}_ms": [round(x, 3) for x in v] for k, v in cases.items()},
                    "nts_fused_us_per_step": round(med["nts_fused"] * 1e3 / args.region, 3),
                    "car_fused_us_per_step": round(med["car_fused"] * 1e3 / args.region, 3),
                    "car_commit_us_per_launch": round(med["car_commit"] * 1e3, 3),
                    "car_over_nts_fused": round(med["car_fused"] / med["nts_fused"], 3),
                    "car_with_commit_over_nts_fused": round((med["car_fused"] + med["car_commit"]) / med["nts_fused"], 3),
                    "records_committed_in_the_regions": [a - b for a, b in zip(counts, counts_before)],
                    "pool_counts": counts, "episodes_nts": nts.stats()["episodes"], "episodes_car": car.stats()["episodes"]}
            fh.write(json.dumps(line) + "\n")
            fh.flush()
            print(json.dumps(line), flush=True)
            del nts, car, env_n, env_c


def train_one(name):
    """train.main in this process, the learner's launches wrapped: boards per stage at every launch boundary"""
    pkg, torch, dev = package()
    import train

    thr = torch.tensor([t.bit_length() - 1 for t in TILES], dtype=torch.uint8, device=dev)
    seen = torch.zeros(len(TILES) + 1, dtype=torch.int64, device=dev)
    real = pkg.BatchedNTupleAgent.fused_rollout

    def wrapped(self, env, steps, *a, **kw):
        r = real(self, env, steps, *a, **kw)
        top = (env.boards.view(env.num_envs, 16) & 15).amax(dim=1)
        seen.add_(torch.bincount((top[:, None] >= thr[None, :]).sum(dim=1), minlength=len(TILES) + 1))
        return r

    pkg.BatchedNTupleAgent.fused_rollout = wrapped
    tag = f"r19_carousel_train_{name}"
    argv = ["--device", args.device.split(":")[0], "--agent", "ntuple", "--num-envs", str(args.num_envs), "--episodes",
            str(args.episodes), "--eval-every", str(args.eval_every), "--seed", str(args.seed), *RUNS[name], "--eval-log",
            out(f"{tag}_eval.jsonl"), "--log", os.devnull, "--save", os.path.join(REPO, args.models, f"carousel_{name}.pt")]
    print("train.py " + " ".join(argv), flush=True)
    with open(out(f"{tag}.log"), "w") as fh, contextlib.redirect_stdout(fh):
        train.main(argv)
    n = seen.cpu().tolist()
    line = {"case": "carousel_stage_share", "run": name, "stage_tiles": list(TILES), "boards_seen_per_stage": n,
            "share_per_stage": [round(x / max(sum(n), 1), 5) for x in n],
            "sampled": "all lanes at every launch boundary of the learner"}
    print(json.dumps(line), flush=True)


def strength():
    mine = sys.argv[1:]
    at = mine.index("--child")
    mine = mine[:at] + mine[at + 2:]                     # this process's own --child goes; the last one given would win
    for name in RUNS:
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "train:" + name]
        r = subprocess.run(cmd + mine, capture_output=True, text=True, cwd=REPO)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:                            # a fault, an abort or a time limit: nothing more is started
            sys.stderr.write(r.stderr[-4000:])
            raise SystemExit(r.returncode)
        with open(out("r19_carousel_stage_share.jsonl"), "w" if name == "plain" else "a") as fh:
            fh.write(r.stdout.strip().splitlines()[-1] + "\n")
        with open(out(f"r19_carousel_train_{name}_eval.jsonl")) as fh:
            last = json.loads(fh.read().strip().splitlines()[-1])
        print(json.dumps({"run": name, **{k: last[k] for k in ("epoch", "games", "mean_score")}}), flush=True)


if args.child:
    if args.child.startswith("train:"):
        train_one(args.child.split(":", 1)[1])
    else:
        {"step_time": step_time, "strength": strength}[args.child]()
    raise SystemExit(0)

os.makedirs(args.out, exist_ok=True)
os.makedirs(os.path.join(REPO, args.models), exist_ok=True)
for step in args.steps:
    limit = args.limit if step == "step_time" else args.limit * 3 + 60    # strength: three runs, each under --limit
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", step] + sys.argv[1:]
    t0 = time.time()
    rc = subprocess.run(cmd).returncode
    print(f"[{step}] exit {rc} after {time.time() - t0:.1f} s", flush=True)
    if rc != 0:                                      # a fault, an abort or a time limit: nothing more is started
        raise SystemExit(rc)
