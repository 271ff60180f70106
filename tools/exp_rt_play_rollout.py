#!/usr/bin/env python3
"""The greedy player on row-tuple weights (q2048_rt_play_rollout) against the loop it replaces, in one process, timed
by HIP events.

For every batch (65 536 and 1 048 576 envs) the weights are trained first by `fused_rollout` at that very size (192
steps), then the same games are played from the boards training left
  loop    by `evaluate.play_legal_moves` on the same agent: per step rt_lookup, legal_moves, env_step, env_reset
          and about twenty torch kernels, one host read per region                      -> "loop_us_per_step"
  fused   by `BatchedRowTupleAgent.play_rollout`: one launch per region                 -> "fused_us_per_step"
in regions of 64 steps, five timed regions each after one untimed, in alternating order (loop first, then fused
first, ...).  The two envs must end on the same boards and aux (epsilon 0: the same games) -- a condition, checked at
every size -- and the weights must be bit-identical afterwards.  Then the COMPANION is timed on the same weights:
`fused_rollout` at lr = 0, which sends the same four 16-byte gathers per step (agent-scope loads there, plain loads in
the player) plus four 4-byte stores the player does not send, and takes no legal-move mask -> "companion_us_per_step"
One JSON line per batch: medians, every region's ms, the ratios loop / fused and fused / companion.
    python tools/exp_rt_play_rollout.py > profiles/r11_rt_play_rollout.jsonl
`--device cpu --sizes 2048` rehearses the script on the CPU twin (host clock; its times say nothing about the GPU)."""
import argparse
import importlib
import json
import os
import sys
import time
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("2048_q-learning_amd")
evaluate = importlib.import_module("evaluate")

p = argparse.ArgumentParser()
p.add_argument("--device", default="cuda:0")
p.add_argument("--sizes", type=int, nargs="+", default=[65536, 1048576])
p.add_argument("--steps", type=int, default=64, help="steps per region")
p.add_argument("--regions", type=int, default=5)
args = p.parse_args()
dev = torch.device(args.device)
on_gpu = dev.type == "cuda"
if on_gpu:
    torch.cuda.set_device(dev)


def timed(fn):
    """ms of fn() on the stream: HIP events around it (the CPU twin: the host clock; every call is synchronous)."""
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


def twin_of(env):
    other = pkg.BatchedGame2048Env(env.num_envs, 4, dev, env.seed, env.env_id0)
    other.load_state_dict(env.state_dict())
    return other


def median(xs):
    return sorted(xs)[len(xs) // 2]


for B in args.sizes:
    env = pkg.BatchedGame2048Env(B, 4, dev, seed=8, env_id0=0)
    agent = pkg.BatchedRowTupleAgent(100, learning_rate=0.1, discount_factor=0.95, exploration_rate=0.3, seed=8,
                                     env_id0=0, device=dev)
    for _ in range(3):
        agent.fused_rollout(env, 64)
    weights = agent.weights.clone()
    env_loop, env_fused = twin_of(env), twin_of(env)
    K = args.steps

    def loop():
        a = types.SimpleNamespace(seed=8, epsilon=0.0, steps_per_launch=K, max_steps=env_loop.ctr + K)
        evaluate.play_legal_moves(torch, agent, env_loop, a, 1 << 62)

    def fused():
        agent.play_rollout(env_fused, K)

    loop(), fused()                                      # untimed: every kernel and torch op of both paths once
    t_loop, t_fused = [], []
    for r in range(args.regions):
        for which in ((loop, fused) if r % 2 == 0 else (fused, loop)):
            (t_loop if which is loop else t_fused).append(timed(which))
    same = bool(torch.equal(env_loop.boards, env_fused.boards) and torch.equal(env_loop.aux, env_fused.aux))
    untouched = bool(torch.equal(weights.view(torch.int32), agent.weights.view(torch.int32)))
    st = agent.play_stats()
    # the companion: the learner's own fused step with nothing to learn (lr = 0, epsilon 0), same weights, same size
    agent.lr, agent.epsilon = 0.0, 0.0
    agent.fused_rollout(env, K)
    t_comp = [timed(lambda: agent.fused_rollout(env, K)) for _ in range(args.regions)]
    us = lambda ms: round(median(ms) * 1e3 / K, 3)       # noqa: E731
    print(json.dumps({
        "case": "rt_play_rollout", "device": str(dev), "board_size": 4, "envs": B, "steps_per_region": K,
        "regions": args.regions, "loop_ms": [round(t, 3) for t in t_loop], "fused_ms": [round(t, 3) for t in t_fused],
        "companion_ms": [round(t, 3) for t in t_comp], "loop_us_per_step": us(t_loop), "fused_us_per_step": us(t_fused),
        "companion_us_per_step": us(t_comp), "loop_over_fused": round(median(t_loop) / median(t_fused), 2),
        "fused_env_steps_per_s": round(B * K / (median(t_fused) * 1e-3), 1),
        "fused_over_companion": round(median(t_fused) / median(t_comp), 3), "same_games": same,
        "weights_untouched": untouched, "games": st["episodes"],
        "valid_move_frac": round(st["valid_moves"] / max(st["steps"], 1), 6),
    }), flush=True)
    assert same, "the fused player and the four-call loop played different games"
    assert untouched, "the player wrote to the weights"
    del env, env_loop, env_fused, agent
    if on_gpu:
        torch.cuda.empty_cache()
