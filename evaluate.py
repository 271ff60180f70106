#!/usr/bin/env python3
"""evaluate.py -- play a trained Q-table without learning.

The reference's README lists an `evaluate.py` ("script per la valutazione e il testing",
README.md:52) that its repository does not contain.  This is that script for the MI355X path: it
loads a learner written by `train.py --save` (a hash table, or -- "kind": "row_tuple" -- the row-tuple learner's
weights, or -- "kind": "line_tuple" -- the line-tuple learner's, or -- "kind": "line_afterstate" -- the afterstate
learner's values, or -- "kind": "ntuple6_afterstate" -- the 6-tuple afterstate network: the file says which, and the
JSON line then carries "agent": "row-tuple" / "line-tuple" / "afterstate" / "ntuple"; `--fused --search` plays the two
afterstate kinds with a one-level expectimax over the spawn, and the line carries "search": 1; `--search-depth 2` makes
it two levels and "search": 2; the greedy players carry "search": 0; a network file with "stage_tiles" is played as
the multi-stage network it is, and the line of every network file carries "stage_tiles", [] for a plain one), plays `--episodes` games per env
with the stored values -- rows are read, nothing is created or written -- and prints one JSON line: games, mean
score / return, max-tile histogram.  Two policies:

  --policy legal (default)   argmax of the stored row over the moves that CHANGE the board (the trial-move
        mask of Deep_QLearning/main_dir/mainDQL_CNN_step2.py:168-174, `q2048_legal_moves`; first maximum wins
        as in np.argmax, a state without a row reads as zeros): what a trained table is worth as a player.
        Batched calls: q_values, legal_moves, step, reset(done).  With --fused the whole step -- lookup, mask,
        choice, env step, statistics, reset -- runs in the kernel, `--steps-per-launch` steps per launch
        (q2048_play_rollout): the same games at --epsilon 0, at the batch sizes the project trains at.
  --policy reference         the agent of Agent/main.py:34-38 with its learning switched off, through the
        fused rollout with Q2048_FLAG_NO_LEARN: argmax over ALL four actions.  The reference's loop relies on
        the update that follows an invalid move (its negative reward sends argmax elsewhere, main.py:43,99);
        with nothing learning, a greedy env repeats an invalid argmax until the >100-repeats rule ends the
        episode (Game2048_env.py:122-127) -- a faithful lr = 0 agent, and a poor measure of the table.

    python train.py --num-envs 65536 --episodes 40 --save models/q_65536x40.pt
    python evaluate.py --model models/q_65536x40.pt --num-envs 65536 --episodes 2
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


SEARCH_KINDS = ("line_afterstate", "ntuple6_afterstate")   # what --search can play: the afterstate families


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--model", required=True, help="file written by train.py --save")
    p.add_argument("--episodes", type=int, default=1, help="games per env (on average)")
    p.add_argument("--num-envs", type=int, default=65536)
    p.add_argument("--epsilon", type=float, default=0.0, help="exploration while evaluating (0 = greedy)")
    p.add_argument("--policy", choices=["legal", "reference"], default="legal",
                   help="legal: argmax over the moves that change the board; reference: the lr = 0 agent (argmax over all four)")
    p.add_argument("--seed", type=int, default=12345, help="evaluation draws (spawns); not the training seed")
    p.add_argument("--device", default="cuda")
    p.add_argument("--steps-per-launch", type=int, default=64)
    p.add_argument("--max-steps", type=int, default=100000, help="stop after this many steps per env at the latest")
    p.add_argument("--env-profile", choices=["shaped", "nopenalty"], default="shaped")
    p.add_argument("--reset-shaping-state", action="store_true")
    p.add_argument("--fused", action="store_true",
                   help="--policy legal in ONE launch per --steps-per-launch steps (q2048_play_rollout: lookup, legal-move "
                        "mask, choice, env step, statistics and reset in the kernel) instead of four library calls and "
                        "about twenty torch kernels per step.  Same games at --epsilon 0; with --epsilon > 0 the "
                        "exploring moves come from the step draws (the player's draw contract), not from torch's generator")
    p.add_argument("--search", action="store_true",
                   help="with --fused, on a file of kind line_afterstate or ntuple6_afterstate: the player looks one level "
                        "ahead -- expectimax over the spawn (q2048_av_search_play_rollout / q2048_nt_search_play_rollout): a "
                        "move is worth its merge score plus the mean, over every cell and tile the spawn can produce, of "
                        "the greedy value of the resulting state")
    p.add_argument("--search-depth", type=int, choices=[1, 2], default=None,
                   help="with --search: levels of expectimax (default 1).  2: the value of a state the spawn leads to is "
                        "the best of ITS searched row (q2048_{av,nt}_search_play_rollout_depth): up to 120 x 120 "
                        "evaluations per move instead of 120")
    args = p.parse_args(argv)
    if args.fused and args.policy != "legal":
        p.error("--fused applies to --policy legal")
    if args.search and not args.fused:
        p.error("--search needs --fused: the one-level search runs in the fused player's kernel only")
    if args.search_depth is not None and not args.search:
        p.error("--search-depth needs --search: it is the depth of that search")
    args.search_depth = (args.search_depth or 1) if args.search else 0      # 0: the greedy player
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch

    pkg = importlib.import_module("2048_q-learning_amd")
    sd = torch.load(args.model, map_location="cpu", weights_only=False)
    if args.search and sd.get("kind") not in SEARCH_KINDS:
        held = sd.get("kind") or "hash_table (a Q-table; the file names no kind)"
        raise SystemExit(f"evaluate.py: --search needs a file of kind {' or '.join(SEARCH_KINDS)} (afterstate values: the "
                         f"search averages the value of the states a spawn leads to); {args.model} holds kind {held}")
    if sd.get("kind") in ("row_tuple", "line_tuple", "line_afterstate", "ntuple6_afterstate"):
        return main_row_tuple(args, torch, pkg, sd)
    n, rows = int(sd["board_size"]), len(sd["q"])
    cap = max(int(sd["capacity_log2"]), 4) if "table" in sd else max(16, (2 * max(rows, 1) - 1).bit_length())
    agent = pkg.BatchedQLearningAgent(1, learning_rate=sd["lr"], discount_factor=sd["gamma"],
                                      exploration_rate=args.epsilon, capacity_log2=cap, seed=args.seed,
                                      device=args.device, board_size=n, placement="plain",
                                      symmetric=bool(sd.get("symmetric", False)))   # (a folded table is read folded)
    agent.load_state_dict(sd)
    agent.seed, agent.ctr, agent.epsilon = args.seed, 0, args.epsilon     # evaluation has its own draws
    agent.stats(reset=True)
    env = pkg.BatchedGame2048Env(args.num_envs, n, args.device, args.seed, agent.env_id0,
                                 profile=args.env_profile, reset_shaping_state=args.reset_shaping_state)
    rows_before = agent.table_size()
    target, t0 = args.episodes * args.num_envs, time.time()
    if args.policy == "legal" and args.fused:
        st = play_fused(agent, env, args, target)
    elif args.policy == "legal":
        st = play_legal_moves(torch, agent, env, args, target)
    else:
        st = agent.stats()
        while st["episodes"] < target and env.ctr < args.max_steps:
            for _ in range(4):
                agent.fused_rollout(env, args.steps_per_launch, learn=False)
            st = agent.stats()
    assert agent.table_size() == rows_before and st["inserts"] == 0      # nothing was learnt
    out = {"model": args.model, "rows": rows_before, "board_size": n, "epsilon": args.epsilon,
           "policy": args.policy, **({"symmetric": True} if agent.symmetric else {}),
           "envs": args.num_envs, "games": st["episodes"], "env_steps": st["steps"],
           "mean_score": st["mean_score"], "mean_return": st["mean_return"],
           "valid_move_frac": st["valid_moves"] / max(st["steps"], 1),
           "max_tile_hist": {str(k): v for k, v in st["max_tile_hist"].items()},
           "best_tile": max(st["max_tile_hist"], default=0),
           "search": args.search_depth, "seconds": round(time.time() - t0, 3)}
    if args.fused:
        out["fused"] = True
    print(json.dumps(out))
    return st


def main_row_tuple(args, torch, pkg, sd):
    """A file of `train.py --agent row-tuple --save`: the same three policies on a `BatchedRowTupleAgent`.  There are no
    rows to count: what must not change is the weights, all 4 MiB, bit for bit.  A file of `--agent line-tuple` (8 MiB,
    "kind": "line_tuple") plays the same way on a `BatchedLineTupleAgent`, a file of `--agent afterstate` (2 MiB,
    "kind": "line_afterstate") on a `BatchedAfterstateAgent` ("agent": "afterstate"), a file of `--agent ntuple`
    (256 MiB, "kind": "ntuple6_afterstate") on a `BatchedNTupleAgent` ("agent": "ntuple")."""
    kind = sd.get("kind")
    cls, name = {"row_tuple": (pkg.BatchedRowTupleAgent, "row-tuple"), "line_tuple": (pkg.BatchedLineTupleAgent, "line-tuple"),
                 "line_afterstate": (pkg.BatchedAfterstateAgent, "afterstate"),
                 "ntuple6_afterstate": (pkg.BatchedNTupleAgent, "ntuple")}[kind]
    stage_tiles = tuple(sd.get("stage_tiles") or ())              # a staged network: the file says so
    extra = {"stage_tiles": stage_tiles} if stage_tiles else {}
    agent = cls(1, learning_rate=sd["lr"], discount_factor=sd["gamma"], exploration_rate=args.epsilon, seed=args.seed,
                device=args.device, **extra)
    agent.load_state_dict(sd)
    agent.seed, agent.ctr, agent.epsilon = args.seed, 0, args.epsilon     # evaluation has its own draws
    agent.stats(reset=True)
    env = pkg.BatchedGame2048Env(args.num_envs, 4, args.device, args.seed, agent.env_id0,
                                 profile=args.env_profile, reset_shaping_state=args.reset_shaping_state)
    before = agent.weights.to("cpu", copy=True)
    target, t0 = args.episodes * args.num_envs, time.time()
    if args.policy == "legal" and args.fused:
        st = play_fused(agent, env, args, target)
    elif args.policy == "legal":
        st = play_legal_moves(torch, agent, env, args, target)
    else:
        agent.lr = 0.0                            # the lr = 0 agent: every delta is +-0 (a trained weight is never -0)
        st = agent.stats()
        while st["episodes"] < target and env.ctr < args.max_steps:
            for _ in range(4):
                agent.fused_rollout(env, args.steps_per_launch)
            st = agent.stats()
    assert torch.equal(before.view(torch.int32), agent.weights.cpu().view(torch.int32))   # nothing was learnt
    out = {"model": args.model, "agent": name, "board_size": 4,
           "epsilon": args.epsilon, "policy": args.policy,
           "envs": args.num_envs, "games": st["episodes"], "env_steps": st["steps"],
           "mean_score": st["mean_score"], "mean_return": st["mean_return"],
           "valid_move_frac": st["valid_moves"] / max(st["steps"], 1),
           "max_tile_hist": {str(k): v for k, v in st["max_tile_hist"].items()},
           "best_tile": max(st["max_tile_hist"], default=0),
           "search": args.search_depth, "seconds": round(time.time() - t0, 3)}
    if args.fused:
        out["fused"] = True
    if kind == "ntuple6_afterstate":
        out["stage_tiles"] = list(stage_tiles)
    print(json.dumps(out))
    return st


def play_fused(agent, env, args, target) -> dict:
    """`play_legal_moves` in one launch per `--steps-per-launch` steps (`play_rollout` of either agent class): the same
    cadence -- the number of finished games is read once per launch -- and, at --epsilon 0, the same games."""
    agent.play_stats(reset=True)
    st = agent.play_stats()
    while st["episodes"] < target and env.ctr < args.max_steps:
        if args.search:
            agent.search_rollout(env, args.steps_per_launch, args.epsilon, depth=args.search_depth)
        else:
            agent.play_rollout(env, args.steps_per_launch, args.epsilon)
        st = agent.play_stats()
    games = max(st["episodes"], 1)
    st.update({"mean_score": st["score_sum"] / games, "mean_return": st["return_sum"] / games})
    return st


def play_legal_moves(torch, agent, env, args, target) -> dict:
    """Greedy over the legal moves, batched: per step one row lookup, one legal-move mask, one env step, one masked
    reset; statistics accumulate on the device and are read once per `--steps-per-launch` steps."""
    dev, B = env.device, env.num_envs
    bit = torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=dev)
    idx = torch.arange(4, device=dev)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    acc = torch.zeros(5, dtype=torch.float64, device=dev)          # games, score, return, valid moves, steps
    hist = torch.zeros(32, dtype=torch.int64, device=dev)
    aux_f = env.aux.view(torch.float32)
    games = 0
    while games < target and env.ctr < args.max_steps:
        for _ in range(args.steps_per_launch):
            q = agent.q_values(env.boards)
            legal = (env.legal_moves()[:, None] & bit[None, :]) != 0
            best = torch.where(legal, q, torch.full_like(q, float("-inf")))
            top = (best == best.max(dim=1, keepdim=True).values) & legal
            action = ((top.cumsum(1) == 1) & top).to(torch.int64).mul(idx).sum(1)      # the first maximum (np.argmax)
            if args.epsilon > 0.0:
                pick = torch.rand(B, 4, generator=gen, device=dev).masked_fill(~legal, -1.0).argmax(1)
                action = torch.where(torch.rand(B, generator=gen, device=dev) < args.epsilon, pick, action)
            valid = legal.gather(1, action[:, None])[:, 0]            # (no legal move: action 0, the game is over)
            _, _, done, _ = env.step(action.to(torch.uint8))
            d = done.to(torch.float64)
            acc += torch.stack([d.sum(), (env.score.to(torch.float64) * d).sum(), (aux_f[:, 1].to(torch.float64) * d).sum(),
                                valid.sum().to(torch.float64), torch.tensor(float(B), dtype=torch.float64, device=dev)])
            hist += torch.bincount(env.max_log2.to(torch.int64)[done], minlength=32)[:32]
            env.reset(done)
        games = int(acc[0].item())
    a, h = acc.cpu().numpy(), hist.cpu().numpy()
    st = agent.stats()
    st.update({"episodes": int(a[0]), "steps": int(a[4]), "valid_moves": int(a[3]),
               "mean_score": float(a[1] / max(a[0], 1.0)), "mean_return": float(a[2] / max(a[0], 1.0)),
               "max_tile_hist": {1 << k: int(v) for k, v in enumerate(h) if v}})
    return st


if __name__ == "__main__":
    main()
