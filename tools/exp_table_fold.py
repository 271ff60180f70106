#!/usr/bin/env python3
"""q2048_table_fold against q2048_table_merge of the same source, on one device, timed by HIP events.

A plain source table of 2^CAP slots (default 2^24 = 512 MiB) is filled with ORBITS random boards, each with MEMBERS of
its eight mirror images present (default 750 000 x 8 = 6.10^6 rows, load 0.36), random values.  Every run then
  1. folds the source into an empty folded table of the same capacity (Q2048_FOLD_MEAN_TRAINED, Q2048_MERGE_ADD,
     w = 1): every orbit creates one row                                                      -> "fold_empty"
  2. merges the same source into an empty table of the same capacity (Q2048_MERGE_ADD, w = 1): every row is created
     -- the streaming pass and the claims without the member lookups                           -> "merge_empty"
  3. folds the source into a table that already holds every orbit's row                        -> "fold_all_combined"
Five runs each, the median is reported; one JSON line per case and a summary.  By request count a full orbit of 8 costs
one streaming pass plus about 14 scattered probes of the source (7 by its leader, and a non-leader stops at the first
present member ahead of it: 1 each); what that costs in time is what this tool is for.
    python tools/exp_table_fold.py [cap_log2=24] [orbits=750000] [members=8] | grep summary > profiles/r09_table_fold.jsonl"""
import importlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("2048_q-learning_amd")
N, A = pkg._native, pkg.agent

cap = int(sys.argv[1]) if len(sys.argv) > 1 else 24
orbits = int(sys.argv[2]) if len(sys.argv) > 2 else 750_000
members = int(sys.argv[3]) if len(sys.argv) > 3 else 8
runs = 5
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
L = N.lib()
assert 1 <= members <= 8 and orbits * members <= 0.6 * (1 << cap)

# the source: `orbits` random boards (cells 0..11: the chance of a board with a stabiliser is negligible and such a
# board only has fewer rows), the first `members` of their images np.rot90(b, g) / np.rot90(np.fliplr(b), g - 4)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
shifts = (4 * torch.arange(16, device=dev, dtype=torch.int64)).reshape(4, 4)
src = pkg.BatchedQLearningAgent(1, capacity_log2=cap, device=dev, board_size=4, placement="plain", freeze_load=None)
left, chunk = orbits, 1 << 20
while left > 0:
    k = min(chunk, left)
    b = torch.randint(0, 12, (k, 4, 4), dtype=torch.int64, device=dev, generator=gen)
    b[:, 0, 0] |= 1                                                      # (no all-empty board: key 0 is the empty slot)
    imgs = [torch.rot90(b, g, dims=(1, 2)) for g in range(4)] + [torch.rot90(b.flip(2), g, dims=(1, 2)) for g in range(4)]
    keys = torch.stack([(x << shifts).sum(dim=(1, 2)) for x in imgs[:members]], dim=1).reshape(-1)
    src.import_rows_device(keys.contiguous(), torch.randn((keys.numel(), 4), device=dev, generator=gen))
    left -= k
    del b, imgs, keys
have = src.recount_rows()
assert src.check_status() == 0
stream = A._stream(dev)
counters = torch.zeros(5, dtype=torch.int64, device=dev)
status = torch.zeros(1, dtype=torch.int32, device=dev)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def fold_into(dst):
    counters.zero_()
    ms = timed(lambda: N.check(L.q2048_table_fold(dst.data_ptr(), cap, src.table.data_ptr(), cap, 1, N.FOLD_MEAN_TRAINED,
                                                  N.MERGE_ADD, 1.0, counters.data_ptr(), status.data_ptr(), stream),
                               "table_fold"))
    return ms, counters.tolist()


def merge_into(dst):
    counters.zero_()
    ms = timed(lambda: N.check(L.q2048_table_merge(dst.data_ptr(), cap, src.table.data_ptr(), cap, 1, N.MERGE_ADD, 1.0,
                                                   counters.data_ptr(), status.data_ptr(), stream), "table_merge"))
    return ms, counters.tolist()


def report(case, ms, extra):
    med = sorted(ms)[len(ms) // 2]
    line = {"case": case, "cap_log2": cap, "rows": have, "members": members, "ms": [round(t, 3) for t in ms],
            "median_ms": round(med, 3), "g_rows_per_s": round(have / med / 1e6, 3)}
    line.update(extra)
    print(json.dumps(line), flush=True)
    return med


dst = torch.zeros((1 << cap, N.SIZEOF_SLOT), dtype=torch.uint8, device=dev)
t_fold, t_merge, t_rmw, n_orbits = [], [], [], 0
for r in range(runs):
    dst.zero_()
    ms, c = fold_into(dst)
    assert c[0] == have and c[1] == c[2] and c[3] == c[4] == 0, c
    n_orbits = c[1]
    t_fold.append(ms)
    ms, c = fold_into(dst)                                               # every orbit's row is there now
    assert c[:5] == [have, n_orbits, 0, n_orbits, 0], c
    t_rmw.append(ms)
    dst.zero_()
    ms, c = merge_into(dst)
    assert c[:4] == [have, have, 0, 0], c
    t_merge.append(ms)
m_fold = report("fold_empty", t_fold, {"orbits": n_orbits, "created": n_orbits})
m_merge = report("merge_empty", t_merge, {"created": have})
m_rmw = report("fold_all_combined", t_rmw, {"orbits": n_orbits, "combined": n_orbits})
print(json.dumps({"case": "summary", "rows": have, "orbits": n_orbits, "members": members, "cap_log2": cap,
                  "fold_empty_ms": round(m_fold, 3), "merge_empty_ms": round(m_merge, 3),
                  "fold_empty_over_merge_empty": round(m_fold / m_merge, 3),
                  "fold_all_combined_over_fold_empty": round(m_rmw / m_fold, 3)}), flush=True)
assert int(status.item()) == 0 and N.claim_timeouts(L) == 0
