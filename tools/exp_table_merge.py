#!/usr/bin/env python3
"""q2048_table_merge against the growth's move (k_table_rehash), on one device, timed by HIP events.

A source table of 2^CAP slots (default 2^28 = 8 GiB) is filled with ROWS pseudo-random rows (default 10^8, load 0.37).
Every run then
  1. maps an empty table of the same capacity from physical chunks (the allocator of growing tables) and MERGES the
     source into it (Q2048_MERGE_ADD, w = 1): every row is created                          -> "merge_empty_chunks"
  2. grows that table to twice the capacity: the library's own move of the very same rows     -> "rehash_move"
     (the two send the same requests per row: 16 or 32 bytes read, one claiming compare-and-swap, two 8-byte stores)
  3. merges the source into an empty table of twice the capacity from the ordinary allocator  -> "merge_empty_plain_2x"
     and into an empty one of the same capacity                                               -> "merge_empty_plain"
  4. merges the source into a table that already holds every one of its keys: each row is read, combined and
     written back, none is created                                                            -> "merge_all_combined"
Five runs each, the median is reported; one JSON line per case.
    python tools/exp_table_merge.py [cap_log2=28] [rows=100000000] [board_size=4] > profiles/r08_table_merge.jsonl"""
import importlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("2048_q-learning_amd")
N, A = pkg._native, pkg.agent

cap = int(sys.argv[1]) if len(sys.argv) > 1 else 28
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
n = int(sys.argv[3]) if len(sys.argv) > 3 else 4
words, runs = (1 if n == 4 else 2), 5
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
L = N.lib()
assert rows <= 0.6 * (1 << cap)

# the source: `rows` distinct random keys with random values, through the agent's own bulk import
src = pkg.BatchedQLearningAgent(1, capacity_log2=cap, device=dev, board_size=n, placement="plain", freeze_load=None)
gen = torch.Generator(device=dev)
gen.manual_seed(1)
left, chunk = rows, 1 << 25
while left > 0:
    k = min(chunk, left)
    keys = torch.randint(-(1 << 62), 1 << 62, (k, words), dtype=torch.int64, device=dev, generator=gen)
    keys |= (-(1 << 63)) if words == 2 else 1
    src.import_rows_device(keys.view(-1) if words == 1 else keys, torch.randn((k, 4), device=dev, generator=gen))
    left -= k
    del keys
have = src.recount_rows()
assert src.check_status() == 0
stream = A._stream(dev)
counters = torch.zeros(4, dtype=torch.int64, device=dev)
status = torch.zeros(1, dtype=torch.int32, device=dev)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def merge_into(ptr, dst_cap):
    counters.zero_()
    ms, _ = timed(lambda: N.check(L.q2048_table_merge(ptr, dst_cap, src.table.data_ptr(), cap, words, N.MERGE_ADD, 1.0,
                                                      counters.data_ptr(), status.data_ptr(), stream), "table_merge"))
    return ms, counters.tolist()


def report(case, ms, extra):
    med = sorted(ms)[len(ms) // 2]
    line = {"case": case, "board_size": n, "src_cap_log2": cap, "rows": have, "ms": [round(t, 3) for t in ms],
            "median_ms": round(med, 3), "g_rows_per_s": round(have / med / 1e6, 3)}
    line.update(extra)
    print(json.dumps(line), flush=True)
    return med


t_merge, t_move = [], []
for r in range(runs):
    owner = A._ChunkedTable(cap, dev, max_capacity_log2=cap + 1)
    ms, c = merge_into(owner.ptr, cap)
    assert c == [have, have, 0, 0] and int(status.item()) == 0, c
    t_merge.append(ms)
    g = owner.grow_begin(cap + 1)
    g.wait()
    ms, bigger = timed(lambda: g.commit(words, stream))
    moved = g.finish()
    assert moved == have
    t_move.append(ms)
    del bigger, g, owner                                  # the family's last table: its memory goes back
m_empty = report("merge_empty_chunks", t_merge, {"dst_cap_log2": cap, "dst_memory": "chunks", "created": have, "combined": 0})
m_move = report("rehash_move", t_move, {"dst_cap_log2": cap + 1, "dst_memory": "chunks"})

for case, dst_cap in (("merge_empty_plain_2x", cap + 1), ("merge_empty_plain", cap)):
    dst, ts = torch.zeros((1 << dst_cap, N.SIZEOF_SLOT), dtype=torch.uint8, device=dev), []
    for r in range(runs):
        dst.zero_()
        ms, c = merge_into(dst.data_ptr(), dst_cap)
        assert c == [have, have, 0, 0], c
        ts.append(ms)
    med = report(case, ts, {"dst_cap_log2": dst_cap, "dst_memory": "plain", "created": have, "combined": 0})
    if dst_cap == cap + 1:
        m_plain_2x = med
    del dst

dst, ts = src.table.clone(), []
for r in range(runs):
    ms, c = merge_into(dst.data_ptr(), cap)
    assert c == [have, 0, have, 0], c
    ts.append(ms)
m_rmw = report("merge_all_combined", ts, {"dst_cap_log2": cap, "dst_memory": "plain", "created": 0, "combined": have})
print(json.dumps({"case": "summary", "board_size": n, "rows": have, "merge_empty_g_rows_per_s": round(have / m_empty / 1e6, 3),
                  "rehash_move_g_rows_per_s": round(have / m_move / 1e6, 3),
                  "merge_empty_over_rehash_move": round(m_empty / m_move, 3),
                  "merge_empty_plain_2x_over_rehash_move": round(m_plain_2x / m_move, 3),
                  "merge_all_combined_g_rows_per_s": round(have / m_rmw / 1e6, 3),
                  "merge_all_combined_over_merge_empty": round(m_rmw / m_empty, 3)}), flush=True)
assert int(status.item()) == 0 and N.claim_timeouts(L) == 0
