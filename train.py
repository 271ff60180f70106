#!/usr/bin/env python3
"""train.py -- the episode loop of the reference (QLearningBase/Agent/main.py:65-115) on MI355X.

The reference's README advertises `python train.py --episodes N --alpha A --gamma G --epsilon E`
(README.md:62-75) but ships no such file: its training loop is the `__main__` block of
Agent/main.py with every hyper-parameter a literal (:67-68).  This script is that loop with the
README flags, in two modes:

  --num-envs 1   the reference loop body, line for line, on the drop-in adapters
                 (Game2048_env / QLearningAgent with the reference's Python types), one CSV row
                 per finished episode with the reference's header (Agent/main.py:71-76).
  --num-envs B   B boards per GPU through the fused rollout kernel (`--steps-per-launch` env
                 steps per launch); epsilon decays once per `B` finished episodes (one "epoch" =
                 one episode per env on average); one CSV row per report interval with the
                 aggregated statistics.  Under torchrun every rank trains its own shard of the
                 env batch and its own Q-table replica; only the statistics are all-reduced.
"""
from __future__ import annotations

import argparse
import csv
import importlib
import importlib.util
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--episodes", type=int, default=1000, help="total episodes (per env on average)")
    p.add_argument("--alpha", type=float, default=0.1, help="learning rate (README.md:66)")
    p.add_argument("--gamma", type=float, default=0.99, help="discount factor (README.md:67)")
    p.add_argument("--epsilon", type=float, default=0.95, help="initial exploration rate (README.md:68)")
    p.add_argument("--epsilon-min", type=float, default=0.01)
    p.add_argument("--num-envs", type=int, default=1, help="boards per GPU")
    p.add_argument("--gpus", type=int, default=1,
                   help="GPUs of this node: with N > 1 and no process group in the environment the script "
                        "starts its own N ranks (one per GPU); under torchrun it joins the given group")
    p.add_argument("--board-size", type=int, default=4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--device", default="cuda",
                   help='"cuda[:i]" (MI355X, the HIP library) or "cpu": the CPU twin (libq2048_host.so: the same C ABI '
                        "compiled for the host from the kernels' own per-lane arithmetic) -- an explicit device, never "
                        "a fallback")
    p.add_argument("--steps-per-launch", type=int, default=64)
    p.add_argument("--capacity-log2", type=int, default=0,
                   help="Q-table slots = 2^n, fixed; 0 (default) = a table that grows like the reference's "
                        "defaultdict, without stopping the loop: it starts at --initial-capacity-log2 slots and "
                        "grows fourfold whenever 0.35 of it is in use (the next table is mapped by a host thread "
                        "while the rollouts go on; the rows move between two launches)")
    p.add_argument("--initial-capacity-log2", type=int, default=0,
                   help="first capacity of the growing table; 0 (default) = 2^30 slots (32 GiB) when that is at most "
                        "an eighth of the free device memory, else the largest power of two that is")
    p.add_argument("--freeze-load", type=float, default=0.5,
                   help="what a table does when it cannot grow any more (--capacity-log2, or the growing table at the "
                        "largest capacity the device holds): once this share of its slots holds rows it takes no new "
                        "rows -- rows that exist keep learning, a state without a row reads as zeros (the defaultdict's "
                        "fresh row, Agent/main.py:16) and its updates are dropped and counted in the Drops column "
                        "(SURVEY 7.3; Q2048_FLAG_NO_NEW_ROWS).  0 = never: the table fills up and slows down by orders "
                        "of magnitude")
    p.add_argument("--growth", choices=["async", "sync"], default="async",
                   help="async (default): growth off the critical path (q2048_table_grow_begin / _commit / _finish); "
                        "sync: the host-synchronous q2048_table_grow (same table, bit for bit)")
    p.add_argument("--verify-every", type=int, default=0,
                   help="batched mode: every N reports also count the table's occupied slots against the rows the "
                        "kernels created (one streaming pass, synchronising).  0 (default): the check runs where it "
                        "is free or needed -- at every growth (on the table left behind), before --save and at the "
                        "end of the run")
    p.add_argument("--strict-td", action="store_true", help="compare-and-swap TD writes (bounded: after 16 lost "
                   "races an update is stored plainly and counted in the statistics)")
    p.add_argument("--deterministic", action="store_true",
                   help="batched mode: reproducible two-phase steps (slower; see deterministic_rollout)")
    p.add_argument("--symmetric", action="store_true",
                   help="batched mode, 4x4, hash-table agent, fused path: SYMMETRY FOLDING (Q2048_FLAG_SYMMETRIC) -- one "
                        "table row for the eight mirror images of a board, keyed by the image with the smallest key; up "
                        "to 8x fewer rows for the same experience, so the table freezes that much later.  Learns a "
                        "different table than without the flag (every row is shared by its images); --save records it "
                        "and evaluate.py / --resume / merge_tables.py follow the file")
    p.add_argument("--agent", choices=["hash", "row-tuple", "line-tuple", "afterstate", "ntuple"], default="hash",
                   help="hash = the reference's whole-board Q-table; row-tuple = BASELINE configs[1]; line-tuple = the "
                        "row-tuple learner with the four columns as features beside the four rows (8 MiB of weights; "
                        "--resume of a row-tuple file promotes it: rows kept, columns start at zero); afterstate = one "
                        "VALUE per line entry (2 MiB), a state judged by the four boards its moves lead to: merge score + "
                        "value of the moved board (BatchedAfterstateAgent; its reward is the raw merge score, so --alpha "
                        "may want another value; no other kind of file resumes into it); ntuple = the afterstate learner "
                        "on a 6-tuple network: four 6-cell patterns read on the eight images of the board, one table per "
                        "pattern shared by the images (256 MiB; BatchedNTupleAgent; no other kind of file resumes into it)")
    p.add_argument("--coherence", action="store_true",
                   help="--agent ntuple only: TEMPORAL-COHERENCE step sizes (q2048_nt_tc_*).  Every weight carries the "
                        "signed sum E and the absolute sum A of its TD errors (512 MiB beside the 256 MiB of weights) and "
                        "learns at --alpha / 32 * min(|E| / A, 1): at full rate while its errors agree in sign, ever "
                        "slower as they cancel.  --save keeps the accumulators; --resume of a plain file starts them at "
                        "zero, and a file that holds them needs this flag")
    p.add_argument("--stage-tiles", default="", metavar="T1[,T2...]",
                   help="--agent ntuple only: a MULTI-STAGE network (q2048_nts_*), one table of weights per stage of the "
                        "game.  Tile values, powers of two, ascending (e.g. 2048 or 2048,8192): a board reads the table of "
                        "the stage its largest tile has reached, 256 MiB per stage.  --save records the tiles; --resume of "
                        "a plain ntuple file splits it (every stage starts as the file); a file with other tiles is "
                        "refused.  Not combined with --coherence")
    p.add_argument("--trace-lambda", type=float, default=None, metavar="L",
                   help="--agent ntuple only: TD(lambda) WITH A TRUNCATED TRACE (q2048_nt_lambda_*).  The TD error of a "
                        "step also moves the last --trace-depth afterstates of the lane's episode, the k-th by L^k of "
                        "the step; an explored move cuts the trace.  L in [0, 1] (0.5 is the usual setting).  --save "
                        "keeps the traces; --resume of a file without them starts them empty.  Not combined with "
                        "--coherence or --stage-tiles")
    p.add_argument("--trace-depth", type=int, default=None, metavar="H",
                   help="with --trace-lambda: how many earlier afterstates a lane remembers, 0..3 (default 3; 0 is the "
                        "plain learner)")
    p.add_argument("--synchronous", action="store_true",
                   help="--agent ntuple only: the SYNCHRONOUS BATCH STEP (q2048_nt_sync_*).  In one step every env is "
                        "evaluated against the same frozen weights, the TD errors that fall on a weight are summed exactly "
                        "and the weight moves once by their mean: a run is a pure function of its arguments and repeats "
                        "bit for bit, on the GPU and on --device cpu with any number of threads.  At most 1048576 envs; "
                        "1 GiB of accumulators, never saved: the file is the plain network's.  Not combined with "
                        "--coherence, --stage-tiles, --carousel or --trace-lambda")
    p.add_argument("--promote-every", type=int, default=None, metavar="N",
                   help="with --stage-tiles: every N epochs, copy what each stage has learned into the entries of the next "
                        "stage that are still zero (agent.promote()).  Default 1; 0 = never")
    p.add_argument("--carousel", type=int, default=None, metavar="P",
                   help="with --stage-tiles: CAROUSEL SHAPING (q2048_car_*).  Episodes start in turn at the beginning of "
                        "every stage, from a pool of up to P boards per stage on which earlier games of this process "
                        "entered that stage (an empty board while a stage's pool is empty).  An episode may then be a "
                        "spliced game; it counts towards the epochs and the epsilon schedule like any other.  --save keeps "
                        "the pool; --resume of a file without one starts it empty, another P is refused")
    p.add_argument("--log", default="debug_log.csv", help="CSV log path (Agent/main.py:71)")
    p.add_argument("--report-every", type=int, default=10, help="launches between CSV rows (batched)")
    p.add_argument("--max-steps", type=int, default=0, help="stop after this many env steps per env (0 = off)")
    p.add_argument("--episode-log", default="", help="batched mode: also write one row per finished "
                   "episode with the reference's columns (Agent/main.py:71-76) + Env to this CSV")
    p.add_argument("--reset-shaping-state", action="store_true",
                   help="opt-in fix of a reference bug: Game2048_env.reset (Game2048_env.py:187-191) keeps "
                        "previous_max and the consecutive-action streak, so an episode ended by the "
                        ">100-repeats rule ends again on its first repeated action; with this flag a reset "
                        "restores them.  Default: the reference's behaviour, bit for bit")
    p.add_argument("--env-profile", choices=["shaped", "nopenalty"], default="shaped",
                   help="shaped = QLearningBase's Game2048_env (the reference's tabular path); nopenalty = "
                        "the DQN path's env (Deep_QLearning/environment/Game2048_nopenalty_env.py: reward = "
                        "merge score or -10, done = game over)")
    p.add_argument("--save", default="", help="write the trained learner (Q-table rows -- or, --agent row-tuple / line-tuple, the "
                   "4 / 8 MiB of weights under \"kind\": \"row_tuple\" / \"line_tuple\" --, epsilon schedule, counters) "
                   "to this file when training ends -- the models/ directory of the reference's README; "
                   "evaluate.py and --resume read it")
    p.add_argument("--resume", default="", help="continue from a file written by --save (same agent arguments): "
                   "the table, the statistics, the epoch counter, epsilon where the saved run left it (the "
                   "schedule's phase limits are rebuilt from this run's --episodes) and, when the batch has "
                   "the saved shape, the boards -- save at epoch k + resume to N trains what N epochs train")
    p.add_argument("--fold", choices=["mean", "mean_trained", "sum", "maxabs"], default="",
                   help="with --resume PLAIN --symmetric: the file holds a PLAIN table; fold it into this run's "
                        "symmetry-folded one (q2048_table_fold: the rows of a board's eight mirror images become one, per "
                        "action the mean over the images with a row / over the images whose entry was ever trained / "
                        "the sum / the entry of largest magnitude).  Schedule, statistics and draw counter resume as "
                        "without it; the saved visit rows are dropped.  Without --fold a plain file is refused")
    p.add_argument("--unfold", action="store_true",
                   help="with --resume FOLDED, without --symmetric: the file holds a SYMMETRY-FOLDED table; unfold it into "
                        "this run's plain one (q2048_table_unfold: every row becomes the rows of its board's eight mirror "
                        "images, each in that image's own frame) -- how a folded file continues under --deterministic or "
                        "in the one-env loop.  Schedule, statistics and draw counter resume as without it; the saved "
                        "visit rows are dropped.  Without --unfold a folded file is refused")
    p.add_argument("--launch-timeout", type=float, default=86400.0,
                   help="self-launched ranks (--gpus N > 1 outside torchrun) are stopped after this many seconds")
    p.add_argument("--stop-epoch", type=int, default=0, help="stop (and --save) once this many epochs of the "
                   "--episodes schedule are done; 0 = run to the end")
    p.add_argument("--summary", default="", help="after the run, write the per-episode log's summary row "
                   "(layout of the reference's plots/summary_statistics_cleaned.csv) to this CSV")
    p.add_argument("--eval-every", type=int, default=0,
                   help="batched mode, either agent: every N epochs measure the learner as a PLAYER -- greedy over the "
                        "moves that change the board (evaluate.py --policy legal --fused, q2048_play_rollout / "
                        "q2048_rt_play_rollout / q2048_lt_play_rollout / q2048_av_play_rollout / q2048_nt_play_rollout) on a "
                        "separate env batch with its own seed, between two training launches on the training stream. "
                        "The table is only read and training's draws, counters and statistics are untouched: the run "
                        "trains what it trains without the flag.  0 (default) = off")
    p.add_argument("--eval-envs", type=int, default=4096, help="envs of the evaluation batch (--eval-every)")
    p.add_argument("--eval-episodes", type=int, default=1, help="games per evaluation env and evaluation (on average)")
    p.add_argument("--eval-log", default="eval_log.jsonl",
                   help="one JSON line per evaluation: epoch, env_steps trained, games, mean_score, mean_return, "
                        "max_tile_hist, valid_move_frac (PATH.rankR in a multi-rank job: every rank plays its replica)")
    p.add_argument("--eval-max-steps", type=int, default=100000, help="an evaluation stops after this many steps per env "
                   "at the latest")
    return p.parse_args(argv)


def log_debug_info(file_path, episode, action, q_values, reward, total_reward, max_value):
    """Agent/main.py:59-62."""
    with open(file_path, mode="a", newline="") as file:
        csv.writer(file).writerow([episode, action, q_values, reward, total_reward, max_value])


def train_single(args, pkg):
    """Agent/main.py:65-115 with the adapters: the loop body below is the reference's."""
    # (play_first_board: the reset before the first episode keeps the constructor's game, so that this loop plays
    # what lane 0 of the batched rollout plays and what the golden transcript G6 recorded -- draw for draw)
    env = pkg.Game2048_env(device=args.device, seed=args.seed, profile=args.env_profile,  # :66
                           reset_shaping_state=args.reset_shaping_state, play_first_board=not args.resume)
    num_episodes = args.episodes                                                       # :67
    agent = pkg.QLearningAgent(num_episodes, action_space=env.action_space.n,          # :68
                               learning_rate=args.alpha, discount_factor=args.gamma,
                               exploration_rate=args.epsilon, exploration_min=args.epsilon_min,
                               capacity_log2=args.capacity_log2 or 22, device=args.device,
                               seed=args.seed)
    first_episode = 0
    if args.resume:
        sd = _load(args.resume, 0)
        if args.unfold:
            _unfold_into(pkg, agent._b, sd, args, agent._b.device)
        else:
            agent._b.load_state_dict(sd)
        first_episode = _resume_schedule(agent._b, sd, args, 1)
    log_file = args.log                                                                # :71
    with open(log_file, mode="w", newline="") as file:                                 # :74-76
        csv.writer(file).writerow(["Episode", "Action", "Q-Values", "Reward", "Total-Reward", "Max Value"])
    max_number_in_train = 0
    t0, steps = time.time(), 0
    stop = min(num_episodes, args.stop_epoch) if args.stop_epoch else num_episodes
    agent._b.train_progress = {"epoch": stop}
    for episode in range(first_episode, stop):                                         # :80
        state = env.reset()                                                            # :81
        state = tuple(map(tuple, state))                                               # :82
        done = False
        total_reward = 0
        max_number_in_train = max(max_number_in_train, int(np.max(env.game.board)))    # :85-86
        while not done:                                                                # :91
            action = agent.choose_action(state)                                        # :92
            next_state, reward, done, info = env.step(action)                          # :93
            next_state = tuple(map(tuple, next_state))                                 # :94
            agent.update_q_value(state, action, reward, next_state, done)              # :99
            q_values = agent.q_table[state]                                            # :96 (post-update alias)
            max_value = np.max(next_state)                                             # :97
            state = next_state                                                         # :100
            total_reward += reward                                                     # :101
            steps += 1
            if done:                                                                   # :103-105
                log_debug_info(log_file, episode, action, q_values, reward, total_reward, max_value)
        agent.decay_exploration(episode)                                               # :109
        if episode % 100 == 0:
            print(f"Episode {episode}: Total Reward: {total_reward} epsilon {agent.epsilon:.4f} "
                  f"rows {len(agent.q_table)} steps/s {steps / (time.time() - t0):.0f}")
    return agent


def train_batched(args, pkg):
    import torch

    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and args.device != "cpu":
        # a rank of a multi-GPU job sits on the CPUs next to ITS GPU -- the device it will really use: the index named
        # by --device cuda:N, else one GPU per local rank (sysfs + sched_setaffinity, no GPU call yet;
        # torch.cuda.device_count() does not initialise the GPU)
        idx = int(args.device.split(":", 1)[1]) if ":" in args.device else (
            int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1))
        pkg.launch.pin_to_gpu_numa_node(idx)
    rank, local_rank, world = pkg.dist.init_process_group()
    if args.device == "cpu":
        dev = torch.device("cpu")
    elif ":" in args.device:
        dev = torch.device(args.device)
    else:       # one rank = one GPU of the node (ranks share GPUs only in rehearsals on a smaller box)
        dev = torch.device("cuda", local_rank % max(torch.cuda.device_count(), 1))
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    shard = pkg.weak_shard(args.num_envs, world, rank)
    B = shard.num_envs
    # the reference's q_table is a defaultdict (Agent/main.py:16): no capacity to choose.  Without
    # --capacity-log2 the device table grows as the run goes (BatchedQLearningAgent(capacity_log2="auto"))
    cap = args.capacity_log2 or "auto"
    env = pkg.BatchedGame2048Env(B, args.board_size, dev, args.seed, shard.env_id0,
                                 profile=args.env_profile, reset_shaping_state=args.reset_shaping_state)
    reducer = pkg.StatsAllReduce(dev)                 # the only collective, on a stream of its own
    if args.agent == "row-tuple":
        agent = pkg.BatchedRowTupleAgent(args.episodes, 4, args.alpha, args.gamma, args.epsilon,
                                         args.epsilon_min, dev, args.seed, shard.env_id0)
    elif args.agent == "line-tuple":
        agent = pkg.BatchedLineTupleAgent(args.episodes, 4, args.alpha, args.gamma, args.epsilon,
                                          args.epsilon_min, dev, args.seed, shard.env_id0)
    elif args.agent == "afterstate":
        agent = pkg.BatchedAfterstateAgent(args.episodes, 4, args.alpha, args.gamma, args.epsilon,
                                           args.epsilon_min, dev, args.seed, shard.env_id0)
    elif args.agent == "ntuple":
        agent = pkg.BatchedNTupleAgent(args.episodes, 4, args.alpha, args.gamma, args.epsilon,
                                       args.epsilon_min, dev, args.seed, shard.env_id0, coherence=args.coherence,
                                       stage_tiles=args.stage_tiles, **({"carousel": args.carousel} if args.carousel else {}),
                                       **({"trace_lambda": args.trace_lambda, "trace_depth": args.trace_depth}
                                          if args.trace_lambda is not None else {}),
                                       **({"synchronous": True} if args.synchronous else {}))
    else:
        agent = pkg.BatchedQLearningAgent(args.episodes, 4, args.alpha, args.gamma, args.epsilon,
                                          args.epsilon_min, cap, dev, args.seed, shard.env_id0,
                                          strict_td=args.strict_td, board_size=args.board_size,
                                          initial_capacity_log2=args.initial_capacity_log2 or "auto",
                                          async_growth=args.growth == "async", freeze_load=args.freeze_load or None,
                                          symmetric=args.symmetric)
    if args.deterministic and args.agent != "hash":
        raise SystemExit("--deterministic applies to the hash-table agent")
    epoch0 = 0
    if args.resume:
        sd = _load(args.resume, rank)
        if args.agent == "ntuple" and sd.get("kind") == "ntuple6_afterstate":
            if "coherence" in sd and not args.coherence:
                raise SystemExit(f"{args.resume} holds temporal-coherence accumulators: resume it with --coherence "
                                 "(without the flag a --save would silently drop them)")
            if args.coherence and "coherence" not in sd and rank == 0:
                print(f"{args.resume} holds no temporal-coherence accumulators: the weights continue, the accumulators "
                      "start at zero (every rate restarts at 1)", flush=True)
            if "trace" in sd and args.trace_lambda is None:
                raise SystemExit(f"{args.resume} holds eligibility traces: resume it with --trace-lambda "
                                 "(without the flag a --save would silently drop them)")
            if args.stage_tiles and not sd.get("stage_tiles") and rank == 0:
                print(f"{args.resume} holds a plain network: every one of the {len(args.stage_tiles) + 1} stages starts "
                      "as the file (stage 0 loaded, the later ones promoted from it)", flush=True)
        if args.fold:
            _fold_into(pkg, agent, sd, args, dev)
        elif args.unfold:
            _unfold_into(pkg, agent, sd, args, dev)
        elif args.agent == "line-tuple" and sd.get("kind") == "row_tuple":
            agent.load_row_tuple(sd)              # promotion: the trained rows go on learning with columns
            if rank == 0:
                print(f"promoted {args.resume}: row-tuple weights into features 0..3, columns start at zero", flush=True)
        else:
            agent.load_state_dict(sd)
        epoch0 = _resume_schedule(agent, sd, args, shard.total_envs)
        env_sd = sd.get("env")
        if env_sd is not None and tuple(env_sd["boards"].shape) == tuple(env.boards.shape) and \
                env_sd["env_id0"] == shard.env_id0 and env_sd["board_size"] == args.board_size:
            env.load_state_dict(env_sd)           # the saved games go on where they stopped
        else:
            env.ctr = agent.ctr                   # fresh boards, the learner's draw counter
    if rank == 0:
        with open(args.log, mode="w", newline="") as fh:
            csv.writer(fh).writerow(["Epoch", "Episodes", "Env-Steps", "Epsilon", "Mean-Return",
                                     "Mean-Score", "Max Value", "Table-Rows", "Drops", "Steps/s"])
    ep_log = None
    if args.episode_log and (args.agent != "hash" or args.deterministic):
        raise SystemExit("--episode-log needs the fused hash-table path")
    if args.episode_log:
        ep_log = pkg.EpisodeLog(max(4 * B, 1 << 16), device=dev)
        ep_path = args.episode_log if world == 1 else f"{args.episode_log}.rank{rank}"
        with open(ep_path, mode="w", newline="") as fh:
            csv.writer(fh).writerow(["Episode", "Action", "Q-Values", "Reward", "Total-Reward",
                                     "Max Value", "Env"])
    # a resumed run goes on from the saved statistics: `epoch` epochs are done, epsilon has been
    # decayed that many times (Agent/main.py:109), the episode count is the restored one
    if args.agent == "hash" and getattr(agent, "_growth", None) is not None:
        # set-up, before the clock starts: the table the first growth moves into is mapped (a host thread of the
        # library has been at it since the agent was built); every later one is mapped while the run goes on
        ms = agent.wait_for_prefetch()
        print(f"[rank {rank}] next table (2^{agent._growth.new_capacity_log2} slots) "
              + (f"mapped in {ms:.0f} ms before the run" if agent._growth.prepared_ok else
                 f"could NOT be mapped ({ms:.0f} ms): the run stays on 2^{agent.capacity_log2} slots"), flush=True)
    total_eps, epoch, launches, t0 = 0, epoch0, 0, time.time()
    if args.resume:
        reducer.start(agent.stats_i, agent.stats_f)
        total_eps = pkg.stats_dict(*reducer.wait())["episodes"]
    stop_epoch = min(args.episodes, args.stop_epoch) if args.stop_epoch else args.episodes
    target = stop_epoch * shard.total_envs
    best_tile, grown, reports, said_frozen = 0, 0, 0, False
    promoted = epoch0 // args.promote_every if args.stage_tiles and args.promote_every else 0
    evaluator = None
    if args.eval_every > 0:
        evaluator = _Evaluator(args, pkg, agent, dev, rank, world, epoch)
    agent.train_progress = {"epoch": epoch}
    agent.train_env = env
    while total_eps < target:
        if args.deterministic:
            agent.deterministic_rollout(env, args.steps_per_launch)
        elif ep_log is not None:
            agent.fused_rollout(env, args.steps_per_launch, episode_log=ep_log)
        else:
            agent.fused_rollout(env, args.steps_per_launch)
        launches += 1
        if ep_log is not None:
            with open(ep_path, mode="a", newline="") as fh:      # log_debug_info, Agent/main.py:59-62
                wr = csv.writer(fh)
                for rec in ep_log.drain():
                    wr.writerow(pkg.EpisodeLog.csv_row(rec) + [int(rec["env_id"])])
        if launches % args.report_every and not args.max_steps:
            continue
        reducer.start(agent.stats_i, agent.stats_f)       # a few hundred bytes, summed over the ranks
        st = pkg.stats_dict(*reducer.wait())
        total_eps = st["episodes"]
        while epoch < total_eps // shard.total_envs and epoch < args.episodes:
            agent.decay_exploration(epoch)                # Agent/main.py:109, once per epoch
            epoch += 1
        if args.stage_tiles and args.promote_every and epoch // args.promote_every > promoted:
            promoted = epoch // args.promote_every                # once per --promote-every epochs reached
            counts = agent.promote()
            if rank == 0:
                print(f"epoch {epoch}: promoted {counts} entries into stages 1..{len(counts)}", flush=True)
        agent.train_progress = {"epoch": epoch}
        if evaluator is not None:
            evaluator.maybe(epoch, st["steps"])
        best_tile = max(st["max_tile_hist"], default=0)
        reports += 1
        if args.agent == "hash":
            # occupied slots == rows the kernels created: every growth checks the table it leaves behind (no extra
            # pass); a full count only when asked for (--verify-every), before --save and at the end of the run
            if args.verify_every and reports % args.verify_every == 0:
                agent.verify_table()
            grown = _report_growths(agent, grown, rank)
            if agent.frozen and not said_frozen:
                said_frozen, f = True, agent.frozen_at
                print(f"[rank {rank}] table frozen at step {f['at_step']}: 2^{f['capacity_log2']} slots hold {f['rows']} "
                      f"rows (load {f['load']:.3f} >= --freeze-load {agent.freeze_load}); no new rows from here on, "
                      "updates of states without a row are dropped and counted", flush=True)
        if rank == 0:
            rate = st["steps"] / (time.time() - t0)
            with open(args.log, mode="a", newline="") as fh:
                csv.writer(fh).writerow([epoch, total_eps, st["steps"], f"{agent.epsilon:.6f}",
                                         f"{st['mean_return']:.4f}", f"{st['mean_score']:.1f}", best_tile,
                                         st["inserts"], st["drops"], f"{rate:.4e}"])
            print(f"epoch {epoch}/{args.episodes} episodes {total_eps} steps {st['steps']} eps "
                  f"{agent.epsilon:.4f} mean return {st['mean_return']:.3f} best tile {best_tile} "
                  f"rows {st['inserts']} drops {st['drops']} {rate:.3e} env-steps/s", flush=True)
        if args.max_steps and env.ctr >= args.max_steps:
            break
    agent.check_status()
    if args.coherence and rank == 0:
        cs = agent.coherence_summary()
        print(f"coherence: {cs['visited']:.6f} of the weights visited, mean rate {cs['mean_rate']:.6f} over them", flush=True)
    if args.agent == "hash":
        check = agent.verify_table()                      # (waits for a growth still in flight and checks it too)
        grown = _report_growths(agent, grown, rank)
        print(f"[rank {rank}] table check passed: {check['rows']} rows == rows created, 2^{check['capacity_log2']} "
              f"slots, load {check['load']:.3f}" + (" (frozen)" if agent.frozen else ""), flush=True)
    # the collectives are over: leave the group in order (a rank that simply exits lets the backend's threads be torn
    # down under it -- an 8-rank gloo job once ended a rank with "terminate called without an active exception")
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        pkg.dist.barrier()
        torch.distributed.destroy_process_group()
    return agent


class _Evaluator:
    """--eval-every: the learner as a greedy player over the legal moves (`play_rollout` of either agent class) on an
    env batch of its own -- its own seed, derived from --seed; its own step counter -- queued on the training stream
    between two training launches.  The player reads the table and writes its env batch and its own statistics:
    the training env, the agent's counters, row cache, statistics and growth bookkeeping never see it."""

    def __init__(self, args, pkg, agent, dev, rank, world, epoch):
        import json

        self._json, self.args, self.agent = json, args, agent
        seed = (args.seed * 6364136223846793005 + 1442695040888963407) & ((1 << 63) - 1)
        self.env = pkg.BatchedGame2048Env(args.eval_envs, args.board_size, dev, seed, rank * args.eval_envs,
                                          profile=args.env_profile, reset_shaping_state=args.reset_shaping_state)
        self.path = args.eval_log if world == 1 else f"{args.eval_log}.rank{rank}"
        self.next_epoch = (epoch // args.eval_every + 1) * args.eval_every
        open(self.path, "w").close()

    def maybe(self, epoch, env_steps):
        """One evaluation, and one line of the log, per multiple of --eval-every that `epoch` has reached."""
        while self.next_epoch <= epoch:
            self.run(self.next_epoch, env_steps)
            self.next_epoch += self.args.eval_every

    def run(self, epoch, env_steps):
        args, agent, env = self.args, self.agent, self.env
        target, last = args.eval_episodes * env.num_envs, env.ctr + args.eval_max_steps
        agent.play_stats(reset=True)
        st = agent.play_stats()
        while st["episodes"] < target and env.ctr < last:
            agent.play_rollout(env, args.steps_per_launch)
            st = agent.play_stats()
        games = max(st["episodes"], 1)
        line = {"epoch": epoch, "env_steps": env_steps, "games": st["episodes"], "mean_score": st["score_sum"] / games,
                "mean_return": st["return_sum"] / games,
                "max_tile_hist": {str(k): v for k, v in st["max_tile_hist"].items()},
                "valid_move_frac": st["valid_moves"] / max(st["steps"], 1)}
        if getattr(agent, "coherence", None) is not None:      # --coherence: the two numbers of coherence_summary()
            cs = agent.coherence_summary()
            line.update({"coherence_visited": cs["visited"], "coherence_mean_rate": cs["mean_rate"]})
        with open(self.path, "a") as fh:
            fh.write(self._json.dumps(line) + "\n")


def _report_growths(agent, grown, rank) -> int:
    while len(agent.growths) > grown:
        g = agent.growths[grown]
        grown += 1
        print(f"[rank {rank}] table grew 2^{g['from_log2']} -> 2^{g['to_log2']} slots at step {g['at_step']}: "
              f"{g['rows']} rows moved in {g['ms']:.1f} ms on the stream"
              + (f", host blocked {g['host_ms']:.1f} ms (the table had been mapped in {g.get('prepare_ms', 0.0):.0f} ms "
                 "by the library's host thread)" if "host_ms" in g else " (host-synchronous)"), flush=True)
    return grown


def _resume_schedule(agent, sd, args, total_envs) -> int:
    """After load_state_dict: how many epochs the saved run had finished, and the epsilon schedule
    of THIS run (phase limits and decay rates from --episodes / --epsilon / --epsilon-min, as the
    constructor computes them, Agent/main.py:25-32) carrying on from the saved epsilon -- the saved
    limits belong to the saved run's --episodes and would pin a longer run to epsilon_min."""
    eps_now = agent.schedule.epsilon
    agent.schedule.__init__(args.episodes, args.epsilon, args.epsilon_min)
    agent.schedule.epsilon = eps_now
    agent.total_epochs = args.episodes
    if "train" in sd:
        return int(sd["train"]["epoch"])
    done = int(sd["stats_i"][1])                      # Q2048_ST_EPISODES: files written before "train" existed
    return min(args.episodes, done // max(total_envs, 1))


def _fold_into(pkg, agent, sd, args, dev):
    """--resume PLAIN --symmetric --fold: everything but the table loads as always (an empty folded table), then the
    file's plain table is loaded into a scratch agent and folded into the run's (BatchedQLearningAgent.fold_from)."""
    import numpy as np

    if sd.get("symmetric", False):
        raise SystemExit(f"--fold: {args.resume} already holds a symmetry-folded table; resume it without --fold")
    if int(sd["flags"]) & 1:
        raise SystemExit(f"--fold: {args.resume} was trained with private rows per env (Q2048_FLAG_INDEPENDENT): its "
                         "keys are salted by env id and do not decode to boards")
    if int(sd["board_size"]) != 4:
        raise SystemExit(f"--fold: {args.resume} has board size {sd['board_size']}; symmetry folding is built for 4 only")
    table = {k: sd[k] for k in ("keys", "q", "table") if k in sd}
    head = {k: v for k, v in sd.items() if k not in ("keys", "q", "table", "visit_rows")}
    head.update({"symmetric": True, "keys": np.zeros((0,), np.uint64), "q": np.zeros((0, 4), np.float32)})
    agent.load_state_dict(head)                   # schedule, statistics, counters; the table starts empty
    rows = len(table["q"]) if "q" in table else 0
    cap = int(sd["capacity_log2"]) if "table" in table else max(16, (2 * max(rows, 1) - 1).bit_length())
    scratch = pkg.BatchedQLearningAgent(1, learning_rate=sd["lr"], discount_factor=sd["gamma"], capacity_log2=cap,
                                        device=dev, board_size=4, placement="plain", freeze_load=None, row_cache=False)
    scratch.load_state_dict({**head, **table, "symmetric": False})
    out = agent.fold_from(scratch, fold=args.fold, mode="add", weight=1.0)
    print(f"folded {args.resume}: {out['read']} plain rows -> {out['created']} rows ({args.fold})", flush=True)


def _unfold_into(pkg, agent, sd, args, dev):
    """--resume FOLDED --unfold: `_fold_into`'s sibling.  Everything but the table loads as always (an empty plain
    table), then the file's folded table is loaded into a scratch symmetric agent and unfolded into the run's
    (BatchedQLearningAgent.unfold_from)."""
    import numpy as np

    if not sd.get("symmetric", False):
        raise SystemExit(f"--unfold: {args.resume} already holds a plain table; resume it without --unfold")
    if int(sd["board_size"]) != 4:
        raise SystemExit(f"--unfold: {args.resume} has board size {sd['board_size']}; symmetry folding is built for 4 only")
    table = {k: sd[k] for k in ("keys", "q", "table") if k in sd}
    head = {k: v for k, v in sd.items() if k not in ("keys", "q", "table", "visit_rows", "symmetric")}
    head.update({"keys": np.zeros((0,), np.uint64), "q": np.zeros((0, 4), np.float32)})
    agent.load_state_dict(head)                   # schedule, statistics, counters; the table starts empty
    rows = len(table["q"]) if "q" in table else 0
    cap = int(sd["capacity_log2"]) if "table" in table else max(16, (2 * max(rows, 1) - 1).bit_length())
    scratch = pkg.BatchedQLearningAgent(1, learning_rate=sd["lr"], discount_factor=sd["gamma"], capacity_log2=cap,
                                        device=dev, board_size=4, placement="plain", freeze_load=None, row_cache=False,
                                        symmetric=True)
    scratch.load_state_dict({**head, **table, "symmetric": True})
    try:
        out = agent.unfold_from(scratch, mode="add", weight=1.0)
    except ValueError as exc:
        raise SystemExit(f"--unfold: {exc} (up to eight rows per row of {args.resume}: raise --capacity-log2)")
    print(f"unfolded {args.resume}: {out['read']} folded rows -> {out['created']} rows", flush=True)


def _load(path, rank):
    import torch

    return torch.load(path if rank == 0 and not os.path.exists(f"{path}.rank0") else f"{path}.rank{rank}",
                      map_location="cpu", weights_only=False)


def _save(agent, path, world, rank):
    """One file per rank (every rank trains its own replica): PATH for a single process, PATH.rankR in a job."""
    import torch

    batched = agent._b if hasattr(agent, "_b") else agent
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    sd = batched.state_dict(compact=True)
    sd["train"] = dict(getattr(batched, "train_progress", {"epoch": 0}))     # epochs finished (resume)
    env = getattr(batched, "train_env", None)
    if env is not None:
        sd["env"] = env.state_dict()                                         # the games in progress
    # (protocol 4: the rows of a long run are numpy arrays of more than 4 GiB -- 5.10^8 rows are 4 GB of keys
    # and 8 GB of values -- which the default protocol of torch.save refuses)
    torch.save(sd, path if world == 1 else f"{path}.rank{rank}", pickle_protocol=4)


def main(argv=None):
    args = parse_args(argv)
    if args.symmetric:
        if args.board_size != 4:
            raise SystemExit("--symmetric folds 4x4 boards only (--board-size 5 is not built)")
        if args.agent != "hash" or args.deterministic:
            raise SystemExit("--symmetric applies to the fused hash-table path (not --agent " +
                             (args.agent if args.agent != "hash" else "row-tuple") + ", not --deterministic)")
        if args.num_envs == 1 and args.gpus == 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1:
            raise SystemExit("--symmetric needs the batched mode (--num-envs > 1): the one-state loop learns through "
                             "choose_action / update_q_value, which do not take the flag")
    try:
        args.stage_tiles = tuple(int(t) for t in args.stage_tiles.split(",") if t.strip())
    except ValueError:
        raise SystemExit(f"--stage-tiles takes tile values separated by commas, not {args.stage_tiles!r}")
    if args.synchronous:
        if args.agent != "ntuple":
            raise SystemExit(f"--synchronous applies to --agent ntuple (the 6-tuple afterstate network), not to --agent {args.agent}")
        for flag, given in (("--coherence", args.coherence), ("--stage-tiles", args.stage_tiles),
                            ("--carousel", args.carousel is not None), ("--trace-lambda", args.trace_lambda is not None)):
            if given:
                raise SystemExit(f"--synchronous is not combined with {flag}: the synchronous batch step is the plain "
                                 "network's")
        if args.num_envs == 1 and args.gpus == 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1:
            raise SystemExit("--synchronous needs the batched mode (--num-envs > 1): the one-state loop runs the hash-table agent")
        if args.num_envs > 1 << 20:
            raise SystemExit("--synchronous sums at most 1048576 envs' errors exactly: fewer --num-envs")
    if args.stage_tiles:
        if args.agent != "ntuple":
            raise SystemExit(f"--stage-tiles applies to --agent ntuple (the 6-tuple afterstate network), not to --agent {args.agent}")
        if args.coherence:
            raise SystemExit("--coherence is not combined with --stage-tiles: the temporal-coherence step knows one table")
        if args.num_envs <= 1:
            raise SystemExit("--stage-tiles needs the batched mode (--num-envs > 1)")
        if any(t < 2 or t > 32768 or t & (t - 1) for t in args.stage_tiles) or \
                any(x >= y for x, y in zip(args.stage_tiles, args.stage_tiles[1:])) or len(args.stage_tiles) > 7:
            raise SystemExit(f"--stage-tiles: at most seven powers of two from 2 to 32768, ascending, not {list(args.stage_tiles)}")
        if args.promote_every is None:
            args.promote_every = 1
        if args.promote_every < 0:
            raise SystemExit("--promote-every counts epochs: 0 (never) or more")
    elif args.promote_every is not None:
        raise SystemExit("--promote-every applies with --stage-tiles")
    if args.carousel is not None:
        if not args.stage_tiles:
            raise SystemExit("--carousel applies with --stage-tiles")
        if args.carousel < 1 or args.carousel > 1 << 32:
            raise SystemExit("--carousel counts the records of a stage's pool: 1 to 2^32")
    if args.trace_lambda is not None:
        if args.agent != "ntuple":
            raise SystemExit(f"--trace-lambda applies to --agent ntuple (the 6-tuple afterstate network), not to --agent {args.agent}")
        if args.coherence or args.stage_tiles:
            raise SystemExit("--trace-lambda is not combined with --coherence or --stage-tiles: the TD(lambda) step knows "
                             "one table and one step size")
        if args.num_envs == 1 and args.gpus == 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1:
            raise SystemExit("--trace-lambda needs the batched mode (--num-envs > 1): the one-state loop runs the hash-table agent")
        if not 0.0 <= args.trace_lambda <= 1.0:
            raise SystemExit(f"--trace-lambda is a number in [0, 1], not {args.trace_lambda}")
        if args.trace_depth is None:
            args.trace_depth = 3
        if not 0 <= args.trace_depth <= 3:
            raise SystemExit(f"--trace-depth is 0, 1, 2 or 3, not {args.trace_depth}")
    elif args.trace_depth is not None:
        raise SystemExit("--trace-depth applies with --trace-lambda")
    if args.coherence:
        if args.agent != "ntuple":
            raise SystemExit(f"--coherence applies to --agent ntuple (the 6-tuple afterstate network), not to --agent {args.agent}")
        if args.num_envs == 1 and args.gpus == 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1:
            raise SystemExit("--coherence needs the batched mode (--num-envs > 1): the one-state loop runs the hash-table agent")
    if args.fold:
        if not args.symmetric:
            raise SystemExit("--fold folds a plain file into a symmetry-folded table: it needs --symmetric")
        if not args.resume:
            raise SystemExit("--fold says how the plain file of --resume is folded: it needs --resume")
    if args.unfold:
        if args.agent != "hash":
            raise SystemExit(f"--unfold unfolds a hash table: not with --agent {args.agent}")
        if args.symmetric:
            raise SystemExit("--unfold unfolds a folded file into a PLAIN table: not together with --symmetric (a "
                             "folded file resumes under --symmetric as it is)")
        if not args.resume:
            raise SystemExit("--unfold says that the file of --resume is symmetry-folded: it needs --resume")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # the parent of the job has made no GPU call: one fresh process per rank (launch.py)
        spec = importlib.util.spec_from_file_location(
            "q2048_launch", os.path.join(REPO, "2048_q-learning_amd", "launch.py"))
        launcher = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(launcher)
        cmd = [sys.executable, os.path.abspath(__file__)] + list(sys.argv[1:] if argv is None else argv)
        raise SystemExit(launcher.launch_ranks(cmd, args.gpus, timeout=args.launch_timeout))
    pkg = importlib.import_module("2048_q-learning_amd")
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    single = args.num_envs == 1 and world == 1
    if args.summary and not single and not args.episode_log:
        raise SystemExit("--summary needs a per-episode log: --episode-log in batched mode")
    agent = train_single(args, pkg) if single else train_batched(args, pkg)
    if args.save:
        _save(agent, args.save, world, rank)
    if args.summary:                               # one row per log, like the reference's aggregate
        episodes_csv = args.log if single else (args.episode_log if world == 1 else f"{args.episode_log}.rank{rank}")
        out = args.summary if world == 1 else f"{args.summary}.rank{rank}"
        pkg.write_summary([pkg.summarize_csv(episodes_csv)], out)
    return agent


if __name__ == "__main__":
    main()
