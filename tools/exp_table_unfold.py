#!/usr/bin/env python3
"""q2048_table_unfold against q2048_table_merge of the rows it produces, on one device, timed by HIP events.

A symmetry-folded source table of 2^SRC_CAP slots (default 2^22 = 128 MiB) is filled with ORBITS canonical keys of
random boards (default 750 000, load 0.18; cells 0..11, so every orbit has its full eight members), random values.
Every run then
  1. unfolds the source into an empty plain table of 2^DST_CAP slots (default 2^24 = 512 MiB; Q2048_MERGE_ADD, w = 1):
     every member creates its row, 6.10^6 rows, load 0.36                                      -> "unfold_empty"
  2. merges the plain table step 1 produced into an empty table of the same capacity (Q2048_MERGE_ADD, w = 1): the
     same rows are created in the destination, by a lane each instead of eight by one lane     -> "merge_empty"
  3. unfolds the source into a table that already holds every member                           -> "unfold_all_combined"
Five runs each, the median is reported; one JSON line per case and a summary.  By request count an orbit of 8 costs
1/8 of the merge's streaming reads and the same eight find-or-creates, issued one after the other by one lane; what
that costs in time is what this tool is for.
    python tools/exp_table_unfold.py [src_cap_log2=22] [dst_cap_log2=24] [orbits=750000] | grep summary > profiles/r10_table_unfold.jsonl"""
import importlib
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("2048_q-learning_amd")
N, A = pkg._native, pkg.agent

src_cap = int(sys.argv[1]) if len(sys.argv) > 1 else 22
dst_cap = int(sys.argv[2]) if len(sys.argv) > 2 else 24
orbits = int(sys.argv[3]) if len(sys.argv) > 3 else 750_000
runs = 5
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
L = N.lib()
assert orbits <= 0.6 * (1 << src_cap) and 8 * orbits <= 0.6 * (1 << dst_cap)

# the source: the canonical images (q2048_canonicalize) of `orbits` random boards, packed into keys
gen = torch.Generator(device=dev)
gen.manual_seed(1)
shifts = 4 * torch.arange(16, device=dev, dtype=torch.int64)
src = pkg.BatchedQLearningAgent(1, capacity_log2=src_cap, device=dev, board_size=4, placement="plain", freeze_load=None,
                                symmetric=True)
left, chunk = orbits, 1 << 20
while left > 0:
    k = min(chunk, left)
    b = torch.randint(0, 12, (k, 16), dtype=torch.uint8, device=dev, generator=gen)
    b[:, 0] |= 1                                                         # (no all-empty board: key 0 is the empty slot)
    canon, _ = src.canonicalize(b)
    keys = (canon.to(torch.int64) << shifts).sum(dim=1)
    src.import_rows_device(keys.contiguous(), torch.randn((k, 4), device=dev, generator=gen))
    left -= k
    del b, canon, keys
have = src.recount_rows()
assert src.check_status() == 0
stream = A._stream(dev)
counters = torch.zeros(6, dtype=torch.int64, device=dev)
status = torch.zeros(1, dtype=torch.int32, device=dev)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def unfold_into(dst):
    counters.zero_()
    ms = timed(lambda: N.check(L.q2048_table_unfold(dst.data_ptr(), dst_cap, src.table.data_ptr(), src_cap, 1, N.MERGE_ADD,
                                                    1.0, counters.data_ptr(), status.data_ptr(), stream), "table_unfold"))
    return ms, counters.tolist()


def merge_into(dst, plain):
    counters.zero_()
    ms = timed(lambda: N.check(L.q2048_table_merge(dst.data_ptr(), dst_cap, plain.data_ptr(), dst_cap, 1, N.MERGE_ADD, 1.0,
                                                   counters.data_ptr(), status.data_ptr(), stream), "table_merge"))
    return ms, counters.tolist()


def report(case, ms, written, extra):
    med = sorted(ms)[len(ms) // 2]
    line = {"case": case, "src_cap_log2": src_cap, "dst_cap_log2": dst_cap, "orbits": have, "rows_written": written,
            "ms": [round(t, 3) for t in ms], "median_ms": round(med, 3), "g_rows_per_s": round(written / med / 1e6, 3)}
    line.update(extra)
    print(json.dumps(line), flush=True)
    return med


plain = torch.zeros((1 << dst_cap, N.SIZEOF_SLOT), dtype=torch.uint8, device=dev)
dst = torch.zeros((1 << dst_cap, N.SIZEOF_SLOT), dtype=torch.uint8, device=dev)
t_unfold, t_merge, t_rmw, written = [], [], [], 0
for r in range(runs):
    plain.zero_()
    ms, c = unfold_into(plain)
    assert c[0] == have and c[1] == 0 and c[2] == c[3] == 8 * have and c[4] == c[5] == 0, c
    written = c[2]
    t_unfold.append(ms)
    ms, c = unfold_into(plain)                                           # every member's row is there now
    assert c == [have, 0, written, 0, written, 0], c
    t_rmw.append(ms)
    dst.zero_()
    ms, c = merge_into(dst, plain)
    assert c[:4] == [written, written, 0, 0], c
    t_merge.append(ms)
m_unfold = report("unfold_empty", t_unfold, written, {"created": written})
m_merge = report("merge_empty", t_merge, written, {"created": written})
m_rmw = report("unfold_all_combined", t_rmw, written, {"combined": written})
print(json.dumps({"case": "summary", "orbits": have, "rows_written": written, "src_cap_log2": src_cap, "dst_cap_log2": dst_cap,
                  "unfold_empty_ms": round(m_unfold, 3), "merge_empty_ms": round(m_merge, 3),
                  "unfold_empty_over_merge_empty": round(m_unfold / m_merge, 3),
                  "unfold_all_combined_over_unfold_empty": round(m_rmw / m_unfold, 3)}), flush=True)
assert int(status.item()) == 0 and N.claim_timeouts(L) == 0
