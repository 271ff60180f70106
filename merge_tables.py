#!/usr/bin/env python3
"""merge_tables.py -- combine the Q-tables of several saved learners into one, on the device.

A multi-GPU job trains one Q-table replica per rank and reduces only the statistics, so
`train.py --save q.pt` in a job writes q.pt.rank0 ... q.pt.rankR.  This script turns them -- or any files written by
`train.py --save`: two seeds, a run resumed on another table -- into the one file `evaluate.py --model` and
`train.py --resume` load.  Every input is loaded into a scratch table and merged into the destination by one streaming
kernel (q2048_table_merge, `BatchedQLearningAgent.merge_from`): at most two tables are resident at a time and no row
travels through a Python dict.

  --mode mean (default)   the average over the K inputs, a state an input never saw counting as the zero row the
                          reference's defaultdict would hold for it (Agent/main.py:16): q = sum_k q_k / K
         sum              q = sum_k q_k
         maxabs           per action the value of largest magnitude (an untrained entry is exactly 0)
         first / last     where inputs share a state, the first / the last input's row wins; other rows are copied

  --fold mean | mean_trained | sum | maxabs
                          the output is a SYMMETRY-FOLDED table (train.py --symmetric): every plain input is folded
                          on its way in -- the rows of a board's eight mirror images become the one row of their
                          canonical image, combined per action by the mean over the images that have a row / over the
                          images whose entry was ever trained / the sum / the entry of largest magnitude
                          (q2048_table_fold, `BatchedQLearningAgent.fold_from`) -- and --mode acts between inputs as
                          before.  Inputs that are folded already merge as they are, so plain and folded files may
                          be mixed.  One plain input with --fold is the converter of a plain file.  Without --fold a
                          mix is refused and nothing is folded.

  --unfold                the output is a PLAIN table: every symmetry-folded input is unfolded on its way in -- each of
                          its rows becomes the rows of its board's eight mirror images (4, 2 or 1 for boards that are
                          their own images), each in that image's own frame (q2048_table_unfold,
                          `BatchedQLearningAgent.unfold_from`) -- and --mode acts between inputs as before.  Plain
                          inputs merge as they are.  One folded input with --unfold is the converter of a folded file:
                          the way to `train.py --deterministic`, the 4-call API and the reference's own loop.  Not
                          together with --fold.

    python train.py --gpus 8 --num-envs 8388608 --episodes 40 --save models/q.pt
    python merge_tables.py --out models/q_merged.pt models/q.pt.rank*
    python evaluate.py --model models/q_merged.pt
    python merge_tables.py --fold mean_trained --out models/q_folded.pt models/q_plain.pt
    python merge_tables.py --unfold --out models/q_plain.pt models/q_folded.pt

Hyper-parameters, epsilon schedule, seed and training progress come from the first input; the statistics vectors are
summed and the draw counter is the largest of the inputs'.  Prints one JSON line.
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

FLAG_INDEPENDENT = 1


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("inputs", nargs="+", help="files written by train.py --save (q.pt.rank0 q.pt.rank1 ...)")
    p.add_argument("--out", required=True, help="the merged learner (loads like any file of train.py --save)")
    p.add_argument("--mode", choices=["mean", "sum", "maxabs", "first", "last"], default="mean")
    p.add_argument("--fold", choices=["mean", "mean_trained", "sum", "maxabs"], default=None,
                   help="write a symmetry-folded table: plain inputs are folded on their way in (see above)")
    p.add_argument("--unfold", action="store_true",
                   help="write a plain table: symmetry-folded inputs are unfolded on their way in (see above)")
    p.add_argument("--device", default="cuda", help='"cuda[:i]", or "cpu" for the host twin of the kernels')
    args = p.parse_args(argv)
    if args.unfold and args.fold is not None:
        p.error("--unfold and --fold exclude each other: the output is either plain or symmetry-folded")
    return args


def _capacity_for(rows: int) -> int:
    """The smallest table that holds `rows` rows at load <= 0.5 (at least 2^16 slots): evaluate.py's own sizing."""
    return max(16, (2 * max(rows, 1) - 1).bit_length())


def main(argv=None):
    args = parse_args(argv)
    import torch

    pkg = importlib.import_module("2048_q-learning_amd")
    t0 = time.time()
    K = len(args.inputs)
    # pass 1, headers only: one board size, shared tables, and an upper bound of the rows the result can hold
    first, rows_in, folded_in, stats_i, stats_f, ctr = None, [], [], None, None, 0
    for path in args.inputs:
        sd = torch.load(path, map_location="cpu", weights_only=False)
        if sd.get("kind") == "row_tuple":
            raise SystemExit(f"{path} holds row-tuple weights, not a hash table: the two kinds do not mix, and averaging "
                             "weight replicas is not built")
        if sd.get("kind") == "line_tuple":
            raise SystemExit(f"{path} holds line-tuple weights, not a hash table: the two kinds do not mix, and averaging "
                             "weight replicas is not built")
        if sd.get("kind") == "line_afterstate":
            raise SystemExit(f"{path} holds afterstate values, not a hash table: the two kinds do not mix, and averaging "
                             "weight replicas is not built")
        if sd.get("kind") == "ntuple6_afterstate":
            raise SystemExit(f"{path} holds a 6-tuple afterstate network, not a hash table: the two kinds do not mix, and "
                             "averaging weight replicas is not built")
        if first is None:
            first = {k: v for k, v in sd.items() if k not in ("keys", "q", "table", "env", "visit_rows")}
        if int(sd["board_size"]) != int(first["board_size"]):
            raise SystemExit(f"{path}: board size {sd['board_size']}, {args.inputs[0]} has {first['board_size']}")
        folded_in.append(bool(sd.get("symmetric", False)))
        if args.fold is None and not args.unfold and folded_in[-1] != folded_in[0]:
            raise SystemExit(f"{path} and {args.inputs[0]}: a symmetry-folded table (train.py --symmetric) and a plain "
                             "one cannot be merged (--fold folds the plain ones, --unfold unfolds the folded ones)")
        if int(sd["flags"]) & FLAG_INDEPENDENT:
            raise SystemExit(f"{path} was trained with private rows per env (Q2048_FLAG_INDEPENDENT): its keys are "
                             "salted by env id and mean nothing in another learner's table")
        rows_in.append(len(sd["q"]) if "q" in sd else int((sd["table"].view(torch.int64).reshape(-1, 4)[:, 0] != 0).sum()))
        stats_i = sd["stats_i"].clone() if stats_i is None else stats_i + sd["stats_i"]
        stats_f = sd["stats_f"].clone() if stats_f is None else stats_f + sd["stats_f"]
        ctr = max(ctr, int(sd["ctr"]))
        del sd
    n = int(first["board_size"])

    def agent_of(capacity_log2, symmetric):
        return pkg.BatchedQLearningAgent(1, learning_rate=first["lr"], discount_factor=first["gamma"],
                                         capacity_log2=capacity_log2, device=args.device, board_size=n,
                                         placement="plain", freeze_load=None, row_cache=False,
                                         symmetric=symmetric)

    if args.fold is not None and n != 4:
        raise SystemExit(f"--fold: symmetry folding is built for board size 4 only, {args.inputs[0]} has {n}")
    if args.unfold and n != 4 and any(folded_in):
        raise SystemExit(f"--unfold: symmetry folding is built for board size 4 only, {args.inputs[0]} has {n}")
    # (--unfold: a folded row becomes up to eight)
    bound = sum(8 * r if args.unfold and f else r for r, f in zip(rows_in, folded_in))
    dst = agent_of(_capacity_for(bound), not args.unfold and (args.fold is not None or folded_in[0]))
    mode, weight = {"mean": ("add", 1.0 / K), "sum": ("add", 1.0), "maxabs": ("maxabs", 1.0),
                    "first": ("blend", 0.0), "last": ("blend", 1.0)}[args.mode]
    merges = []
    for path, rows, folded in zip(args.inputs, rows_in, folded_in):
        sd = torch.load(path, map_location="cpu", weights_only=False)
        sd.pop("visit_rows", None)                    # (the envs' visit rows belong to the run, not to the table)
        scratch = agent_of(int(sd["capacity_log2"]) if "table" in sd else _capacity_for(rows), folded)
        scratch.load_state_dict(sd)
        del sd
        if dst.symmetric and not folded:              # (--fold: a plain input enters through its orbits)
            merges.append(dst.fold_from(scratch, fold=args.fold, mode=mode, weight=weight))
        elif folded and not dst.symmetric:            # (--unfold: a folded input enters through its images)
            merges.append(dst.unfold_from(scratch, mode=mode, weight=weight))
        else:
            merges.append(dst.merge_from(scratch, mode=mode, weight=weight))
        if dst.on_gpu:
            torch.cuda.synchronize(dst.device)
        del scratch                                   # at most two tables at a time
    check = dst.verify_table()
    out = dst.state_dict(compact=True)
    out.update(first)                                 # hyper-parameters, schedule, seed, progress: the first input's
    out.update({"capacity_log2": dst.capacity_log2, "stats_i": stats_i, "stats_f": stats_f, "ctr": ctr,
                "merged": {"inputs": [os.path.basename(p) for p in args.inputs], "mode": args.mode}})
    if args.unfold:
        out.pop("symmetric", None)                    # (the first input's, if that one was folded)
        out["merged"]["unfolded_inputs"] = [os.path.basename(p) for p, f in zip(args.inputs, folded_in) if f]
    if args.fold is not None:
        out["symmetric"] = True
        out["merged"].update({"fold": args.fold, "folded_inputs": [os.path.basename(p) for p, f in
                                                                  zip(args.inputs, folded_in) if not f]})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    torch.save(out, args.out, pickle_protocol=4)      # (protocol 4: rows of a long run pass 4 GiB, as train.py --save)
    report = {"out": args.out, "mode": args.mode, "device": args.device, "board_size": n, "inputs": args.inputs,
              "rows_in": rows_in, "merges": merges, "rows_out": check["rows"],
              "capacity_log2": dst.capacity_log2, "seconds": round(time.time() - t0, 3)}
    if args.fold is not None:
        report["fold"] = args.fold
    if args.unfold:
        report["unfold"] = True
    print(json.dumps(report))
    return out


if __name__ == "__main__":
    main()
