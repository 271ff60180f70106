"""Tabular Q-learning agent on MI355X: the host-side mirror of QLearningBase/Agent/main.py
(class QLearningAgent, :14-57).

`BatchedQLearningAgent` keeps the reference's constructor arguments and method names
(`choose_action`, `update_q_value`, `decay_exploration`, `q_table[state]`, `epsilon`) over B
states at once, with the Q-table as a device open-addressed hash table; `fused_rollout` is the
throughput entry point (whole loop body of Agent/main.py:91-101 in one launch).
`QLearningAgent` is the one-state adapter with the reference's Python types."""
from __future__ import annotations

import ctypes as C
import os
import warnings
import weakref

import numpy as np
import torch

from . import _native as N
from .env import (BatchedGame2048Env, _host_zeros, _ptr, _require_gpu, _Staging, _stream, raw_to_boards,
                  state_to_log2)


class EpsilonSchedule:
    """QLearningAgent's exploration schedule (Agent/main.py:15-32, 45-57), host scalars.
    Same arithmetic in the same order as the reference, so the values are bit-identical."""

    def __init__(self, total_epochs, exploration_rate=1.0, exploration_min=0.01):
        self.epsilon = exploration_rate                                        # :19
        self.epsilon_min = exploration_min                                     # :20
        self.total_epochs = total_epochs                                       # :22
        self.first_decay_limit = total_epochs * 0.30                           # :25
        self.second_decay_limit = total_epochs * 0.60                          # :26
        self.third_decay_limit = total_epochs * 0.80                           # :27
        self.slow_decay_1 = (exploration_rate - (exploration_min * 1.5)) / self.first_decay_limit
        self.fast_decay = ((exploration_rate - exploration_min) - (exploration_min * 1.5)) / (
            self.second_decay_limit - self.first_decay_limit)                  # :31
        self.slow_decay_2 = (exploration_min * 1.1 - exploration_min) / (
            self.third_decay_limit - self.second_decay_limit)                  # :32

    def decay_exploration(self, current_epoch):
        if current_epoch < self.first_decay_limit:                             # :46
            self.epsilon = max(self.epsilon_min * 1.5, self.epsilon - self.slow_decay_1)
        elif current_epoch < self.second_decay_limit:                          # :49
            self.epsilon = max(self.epsilon_min * 1.1, self.epsilon - self.fast_decay)
        elif current_epoch < self.third_decay_limit:                           # :52
            self.epsilon = max(self.epsilon_min, self.epsilon - self.slow_decay_2)
        else:
            self.epsilon = self.epsilon_min                                    # :57


EPISODE_DTYPE = np.dtype([("env_id", "<u8"), ("episode", "<u4"), ("action", "u1"), ("max_log2", "u1"),
                          ("steps_lo", "<u2"), ("reward", "<f4"), ("total_return", "<f4"),
                          ("score", "<i4"), ("q", "<f4", (4,)), ("reserved", "<u4")])


class EpisodeLog:
    """Device buffer of finished-episode records (q2048_episode): the batched form of the rows
    log_debug_info appends to debug_log.csv (Agent/main.py:59-62)."""

    def __init__(self, capacity: int, device="cuda"):
        self.device = _require_gpu(device)
        self.capacity = int(capacity)
        self.records = torch.zeros((self.capacity, N.SIZEOF_EPISODE), dtype=torch.uint8, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)

    def drain(self) -> np.ndarray:
        """Host copy of the records written so far (arrival order), then empties the log.
        `lost` = episodes that finished while the buffer was full."""
        n = int(self.count.item())
        self.lost = max(0, n - self.capacity)
        rec = self.records[: min(n, self.capacity)].cpu().numpy().view(EPISODE_DTYPE).reshape(-1).copy()
        self.count.zero_()
        return rec

    @staticmethod
    def csv_row(rec) -> list:
        """One record in the reference's column order (Agent/main.py:62)."""
        return [int(rec["episode"]), int(rec["action"]), np.asarray(rec["q"], dtype=np.float64),
                float(rec["reward"]), float(rec["total_return"]), 1 << int(rec["max_log2"])]


class _QTableView:
    """`agent.q_table[state]` (Agent/main.py:16,96): state = tuple of 4 tuples of raw tile
    values; returns the 4 Q-values as float64 (zeros when the state was never updated)."""

    def __init__(self, agent: "BatchedQLearningAgent"):
        self._a = weakref.proxy(agent)  # no reference cycle: the table frees with the agent

    def __getitem__(self, state) -> np.ndarray:
        n = self._a.board_size
        b = torch.from_numpy(raw_to_boards(np.asarray(state).reshape(1, n, n))).to(self._a.device)
        return self._a.q_values(b, env_id=self._a.env_id0)[0].double().cpu().numpy()

    def __len__(self) -> int:
        return self._a.table_size()


def _probe_us(table: torch.Tensor, capacity_log2: int, device: torch.device) -> float:
    """us per 2^20 scattered atomics of q2048_table_probe on `table` (contents unchanged)."""
    L, stream, lanes, steps = N.lib(), _stream(device), 1 << 20, 16
    N.check(L.q2048_table_probe(_ptr(table), capacity_log2, lanes, steps, 7, stream), "q2048_table_probe")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for r in range(2):
        N.check(L.q2048_table_probe(_ptr(table), capacity_log2, lanes, steps, 1000 + r, stream),
                "q2048_table_probe")
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (2 * steps)


class _ChunkedTable:
    """Owner of one q2048_table_reserve allocation (a table mapped from small physical chunks that may
    grow up to `max_capacity_log2`: `grow`), handed to torch through __cuda_array_interface__: the
    tensor keeps this object alive, and the memory goes back to the device when the last reference is
    dropped."""

    def __init__(self, capacity_log2: int, device: torch.device, chunk_bytes: int = 0,
                 max_capacity_log2: int | None = None, _adopt: int | None = None):
        self.capacity_log2 = int(capacity_log2)
        self.max_capacity_log2 = int(max_capacity_log2 or capacity_log2)
        self.device = device
        if _adopt is None:
            ptr = C.c_void_p()
            with torch.cuda.device(device):
                N.check(N.lib().q2048_table_reserve(self.capacity_log2, self.max_capacity_log2, chunk_bytes,
                                                    C.byref(ptr)), "q2048_table_reserve")
            _adopt = int(ptr.value)
        self.ptr = _adopt
        self.__cuda_array_interface__ = {"shape": (1 << self.capacity_log2, N.SIZEOF_SLOT), "typestr": "|u1",
                                         "data": (self.ptr, False), "version": 2, "strides": None}
        self._finalizer = weakref.finalize(self, _ChunkedTable._free, self.ptr)

    @staticmethod
    def _free(ptr: int) -> None:
        try:
            N.lib().q2048_table_free(ptr)       # synchronises the table's own device, whatever the current one is
        except Exception:                       # interpreter shutdown: the process's memory goes anyway
            pass

    def tensor(self, device: torch.device) -> torch.Tensor:
        t = torch.as_tensor(self, device=device)
        if t.data_ptr() != self.ptr or t.dtype != torch.uint8:
            raise RuntimeError("torch did not adopt the chunked table in place")
        return t

    def grow(self, new_capacity_log2: int, key_words: int, stream) -> "tuple[_ChunkedTable, int]":
        """q2048_table_grow (host-synchronous): the table of the next capacity, every row moved over, this one
        released (its tensor must not be used again).  Returns (owner of the bigger table, rows moved)."""
        ptr, moved = C.c_void_p(), C.c_int64(0)
        N.check(N.lib().q2048_table_grow(self.ptr, self.capacity_log2, int(new_capacity_log2), key_words,
                                         C.byref(ptr), C.byref(moved), stream), "q2048_table_grow")
        self._finalizer.detach()                # the library released this table's chunks itself
        return _ChunkedTable(new_capacity_log2, self.device, max_capacity_log2=self.max_capacity_log2,
                             _adopt=int(ptr.value)), int(moved.value)

    def grow_begin(self, new_capacity_log2: int) -> "_Growth":
        """q2048_table_grow_begin: the library's host thread starts mapping the bigger table; returns at once."""
        return _Growth(self, int(new_capacity_log2))


class _Growth:
    """One q2048_table_grow_begin .. _commit .. _finish (or _abort): a growth off the caller's critical path.
    Keeps the old table's owner alive until the library has released that table."""

    def __init__(self, owner: _ChunkedTable, new_capacity_log2: int):
        self.owner, self.new_capacity_log2 = owner, new_capacity_log2
        self.handle, self.bigger, self.info, self.prepared_ok = C.c_void_p(), None, {}, None
        with torch.cuda.device(owner.device):
            N.check(N.lib().q2048_table_grow_begin(owner.ptr, owner.capacity_log2, new_capacity_log2,
                                                   C.byref(self.handle)), "q2048_table_grow_begin")

    def ready(self) -> bool:
        """True when the next call (commit, or finish after the commit) will not block."""
        return N.lib().q2048_table_grow_poll(self.handle) != N.PENDING   # (a failure is "ready": the next call reports it)

    def wait(self) -> float:
        """q2048_table_grow_wait: blocks until the bigger table is mapped; returns the ms the host thread spent on
        it (a failure is left for `commit` to report)."""
        ms = C.c_double(0.0)
        self.prepared_ok = N.lib().q2048_table_grow_wait(self.handle, C.byref(ms)) == N.OK
        return float(ms.value)

    def commit(self, key_words: int, stream, verify_count: bool = False) -> _ChunkedTable:
        """q2048_table_grow_commit: the move is queued on `stream`; the bigger table is the table from here on."""
        ptr = C.c_void_p()
        with torch.cuda.device(self.owner.device):
            N.check(N.lib().q2048_table_grow_commit(self.handle, key_words, N.GROW_VERIFY_COUNT if verify_count else 0,
                                                    C.byref(ptr), stream), "q2048_table_grow_commit")
        self.bigger = _ChunkedTable(self.new_capacity_log2, self.owner.device,
                                    max_capacity_log2=self.owner.max_capacity_log2, _adopt=int(ptr.value))
        return self.bigger

    def finish(self) -> int:
        """q2048_table_grow_finish: waits for the move, checks it, hands the old table to the library's host
        thread for release.  Returns the rows moved (= the occupied slots of the old table)."""
        moved = C.c_int64(0)
        code = N.lib().q2048_table_grow_finish(self.handle, C.byref(moved))
        if code == N.OK:
            self.owner._finalizer.detach()      # the library releases the old table itself
        N.check(code, "q2048_table_grow_finish")
        return int(moved.value)

    def abort(self) -> None:
        N.check(N.lib().q2048_table_grow_abort(self.handle), "q2048_table_grow_abort")


def _ranks_on_this_device() -> int:
    """How many ranks of this job run on each GPU (1 on a real multi-GPU node)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    return max(1, -(-world // max(torch.cuda.device_count(), 1)))


def place_table(capacity_log2: int, device: torch.device, placement="auto", max_capacity_log2: int | None = None,
                candidates: int | None = None):
    """Allocate the zeroed table where scattered writes run fast.

    How a multi-GiB table's memory was obtained moves the scattered store / atomic rate of the
    rollout by 15-20 % (DESIGN.md 4 "table placement"; loads do not care): a hipMalloc of 8-32 GiB
    comes back in a slow or a fast state depending on where it lands, small ones nearly always slow,
    while the same table mapped from 2 MiB physical chunks (q2048_table_alloc: HIP virtual-memory
    API) measures as fast as one that spans 128 GiB, on every box so far.  `placement`:
      "auto"    tables of 1..64 GiB: "chunks"; smaller ones (cache-resident) and 128 GiB ones (fast as
                they come: 42.4 us per step from hipMalloc, 42.7 from chunks, four processes each on one
                box; a 64 GiB hipMalloc took 44.3 once and 49.4 three times, chunks 43.6-44.3) "plain"
      "chunks"  q2048_table_alloc: 2 MiB physical chunks mapped into one virtual range (the fastest of
                up to four such tables, as many as fit in half of the free memory together)
      "plain"   torch.zeros (caching allocator -> hipMalloc): whatever the device yields
      n (int)   allocate up to n plain candidates at once, time q2048_table_probe on each (~2 ms,
                contents untouched), keep the fastest, release the others
    `max_capacity_log2` ("chunks" only): the table may grow up to that capacity
    (`BatchedQLearningAgent.grow_table`).  `candidates` ("chunks" only): how many tables to map and probe at most
    (default: up to four on a device of one rank, ONE in a multi-rank job -- eight ranks each mapping 4 x 32 GiB at
    start-up are 8 x 1.2 s of driver calls for a <= 7 % effect -- and one for a table that will grow: it is replaced
    at its first growth anyway, and memory released moments before is what makes the next mapping slow).
    Returns (table, report); report["probe_us"] lists the probe's time on every candidate tried."""
    shape = (1 << capacity_log2, N.SIZEOF_SLOT)
    nbytes = N.SIZEOF_SLOT << capacity_log2
    if placement == "auto":
        if (1 << 30) <= nbytes <= (64 << 30):
            try:
                return place_table(capacity_log2, device, "chunks", max_capacity_log2, candidates)
            except (N.NativeError, RuntimeError) as exc:      # no virtual-memory API on this stack, or no room:
                table = torch.zeros(shape, dtype=torch.uint8, device=device)   # the slower kind of table
                return table, {"mode": "plain", "chunks_failed": str(exc)}
        placement = "plain"
    if placement == "plain":
        return torch.zeros(shape, dtype=torch.uint8, device=device), {"mode": "plain"}
    if placement == "chunks":
        # up to four candidates when the device has the room: chunked tables differ less than hipMalloc'd
        # ones, but on some boxes every second one still probes 10-15 % slower than the rest (57-59 against
        # 49-51 us on 2^28 and 2^30 slots); each candidate costs its mapping + zero-fill (~0.3 s for 32 GiB)
        # (ranks that share one device -- rehearsals of a multi-GPU job on a one-GPU box -- share its free memory)
        free, _ = torch.cuda.mem_get_info(device)
        if candidates is None:
            world = int(os.environ.get("WORLD_SIZE", "1"))
            candidates = 1 if (world > 1 or (max_capacity_log2 or capacity_log2) > capacity_log2) else 4
        tries = int(max(1, min(int(candidates), (0.5 * free / _ranks_on_this_device()) // nbytes)))
        tables, times = [], []
        for _ in range(tries):
            try:
                owner = _ChunkedTable(capacity_log2, device, max_capacity_log2=max_capacity_log2)
                t = owner.tensor(device)
                t._q2048_owner = owner                  # how grow_table finds the allocation again
            except N.NativeError:
                if not tables:
                    raise
                break                                   # the memory went elsewhere meanwhile: keep what there is
            tables.append(t)
            times.append(_probe_us(t, capacity_log2, device))
            del t, owner
        chosen = int(np.argmin(times))
        table = tables[chosen]
        del tables
        return table, {"mode": "chunks", "chunk_bytes": 2 << 20, "candidates": tries, "chosen": chosen,
                       "probe_us": [round(x, 2) for x in times]}
    candidates = int(placement)
    if candidates < 1:
        raise ValueError("placement must be 'auto', 'chunks', 'plain' or a candidate count >= 1")
    tables, times = [], []
    for _ in range(candidates):
        try:
            t = torch.zeros(shape, dtype=torch.uint8, device=device)
        except torch.OutOfMemoryError:
            if not tables:
                raise
            break
        tables.append(t)
        times.append(_probe_us(t, capacity_log2, device))
    chosen = int(np.argmin(times))
    table = tables[chosen]
    del tables, t
    torch.cuda.empty_cache()                                         # give the other candidates back
    return table, {"mode": "candidates", "candidates": len(times),
                   "probe_us": [round(x, 2) for x in times], "chosen": chosen}


def auto_capacity_log2(min_rows: int, device, max_log2: int = 33, floor_log2: int = 30,
                       memory_fraction: float = 0.25) -> int:
    """Table size for a run that will create up to `min_rows` rows: load factor <= 0.5, and not
    below 2^`floor_log2` slots (32 GiB) when that fits in `memory_fraction` of the free device
    memory.  Why a floor: a 2^30-slot table mapped from 2 MiB chunks (`place_table`) runs the rollout
    as fast as one that spans 128 GiB (0.331 against 0.327 of the roofline on the driver's bench
    command), a 2^28-slot one 6 % slower even so -- smaller footprints take scattered atomics more
    slowly on this memory system -- and memory is what an MI355X has plenty of.
    Round 2 took half of the device (2^32 slots) for the same speed."""
    need = max(20, int(np.ceil(np.log2(2.0 * max(int(min_rows), 1)))))
    free, _ = torch.cuda.mem_get_info(torch.device(device))
    fit = int(np.floor(np.log2(max(memory_fraction * free / N.SIZEOF_SLOT, 2.0))))
    return min(max(need, min(fit, floor_log2, max_log2)), 40)


class BatchedQLearningAgent:
    """QLearningAgent over a batch.  Constructor arguments as Agent/main.py:15; extra keyword
    arguments size and place the device table.

    capacity_log2   an int: the table has 2**capacity_log2 slots of 32 B, fixed at construction; when an
                    update finds no free slot within the probe limit it is dropped and counted
                    (stats['drops'], status TABLE_FULL) -- never an exception.
                    "auto": a table that GROWS, like the reference's defaultdict (Agent/main.py:16), without
                    stopping the loop.  It starts at 2**initial_capacity_log2 slots ("auto": 2^30 = 32 GiB when
                    that is at most an eighth of the free device memory, else the largest power of two that is,
                    at least 2^20) and, between launches, grows by a factor 2**growth_step_log2 (4) whenever the
                    rows it holds pass `load_limit` of its capacity (0.35: on a pre-filled table the step costs
                    46 us at load 0.1, 57 at 0.36, 69 at 0.51, 87 at 0.61 -- profiles/r05_load_curve_prefilled.jsonl
                    -- and memory is what the device has plenty of): the next table is mapped by the
                    library's host thread while rollouts go on (`prefetch_growth`: started as soon as the current
                    table is in place; else at half the limit), the move of the rows is queued on the stream
                    between two launches, the check (rows moved == rows the kernels created) and the release of
                    the old table happen later, off the critical path (q2048_table_grow_begin / _commit /
                    _finish).  Up to the largest capacity the device has room for next to its predecessor
                    (2^32 slots = 128 GiB on an MI355X); `growths` lists what happened.  No update is dropped in
                    any run that fits the device.  If the device has no virtual-memory API or no room for the
                    first table the agent falls back to ONE fixed plain table (a warning says so).
                    `async_growth=False`: the host-synchronous q2048_table_grow of round 4 instead (same result,
                    bit for bit: tested).
    freeze_load     what a table does when it CANNOT grow any more (a fixed `capacity_log2`, or a growing one at its
                    largest capacity) -- SURVEY 7.3's "stop inserting and count drops", the device counterpart of a
                    defaultdict (Agent/main.py:16) that has no limit: once the table holds `freeze_load` of its
                    capacity in rows (checked between launches with the kernels' own insert counter, so the load ends
                    within one launch of the limit), every launch carries Q2048_FLAG_NO_NEW_ROWS: rows that exist keep
                    learning, a state without a row reads as the zero row the defaultdict would have created, is not
                    created, and its update is dropped and counted (stats['drops']) -- landing in the env's VISIT ROW,
                    which stands in for the missing row while the env stays in that state (so that an invalid move
                    teaches the next greedy choice, as the defaultdict's fresh row would) and ends when it moves on;
                    a warning says so once and `frozen` is True from then on.  Default 0.5: a 1 Mi-board step on a
                    table frozen there costs what the young learning table's costs (4x4: 47.3 us against 45.5; 5x5:
                    61.4 against 61.5), at 0.6 it is
                    65.9 / 85.5 us, at 0.7 101 / 140, at 0.9 823 / 1206 (profiles/r06_load_curve_frozen*.jsonl), and a
                    table driven to load 1.0 takes 12.9 ms (profiles/r05_claim_first_ab.jsonl).  None: never freeze --
                    the table fills up, probes of absent states walk up to 2^10 slots, and updates that find no slot
                    are dropped (status TABLE_FULL).
    independent     every env owns private rows (keys salted with its global id): B independent
                    learners in one table, exactly B reference agents side by side.
    placement       how the table is allocated (`place_table`): "auto", "chunks", "plain" or a count
                    of candidate allocations to probe.  `self.placement` is the report.
    strict_td       update Q[s][a] with a compare-and-swap loop (concurrent updates of one entry
                    serialise) instead of one store (last writer wins).  Same result whenever
                    no two lanes share (s, a); several times slower when many lanes do.
    symmetric       SYMMETRY FOLDING (Q2048_FLAG_SYMMETRIC, 4x4 only): the table holds one row for the eight mirror
                    images of a board -- four quarter turns, each with or without a mirror -- keyed by the image
                    with the smallest key, and every row learns from all eight images: up to 8x fewer rows for the
                    same experience, so `freeze_load` binds that much later.  `fused_rollout`, `play_rollout`,
                    `q_values`, statistics, growth, freezing, checkpoints and `merge_from` work as without it;
                    everything the caller sees (actions, `q_values`, the episode log) is in the env's own frame.
                    `export_rows` / `export_dict` return the CANONICAL states only (one per orbit;
                    `export_dict(unfold=True)` returns every image, and a plain agent's `unfold_from` takes the
                    whole table over, for the paths that only understand plain tables).  The 4-call API
                    (`choose_action`, `update_q_value`) and `deterministic_rollout` raise ValueError; a folded
                    checkpoint loads only into a folded agent (and a plain one only into a plain agent).
    row_cache       `choose_action` / `update_q_value` hand the row an env read as next_state on to
                    its next call through a device buffer of 32 B per env (q2048_*_cached: what the
                    fused rollout carries in registers), so an update reads one scattered row instead
                    of two.  Used only on a key match, so any calling pattern is correct."""

    def __init__(self, total_epochs, action_space=4, learning_rate=0.1, discount_factor=0.9,
                 exploration_rate=1.0, exploration_min=0.01, capacity_log2: int = 24,
                 device="cuda", seed: int = 0, env_id0: int = 0, independent: bool = False,
                 strict_td: bool = False, board_size: int = 4, placement="auto", row_cache: bool = True,
                 initial_capacity_log2="auto", max_capacity_log2: int | None = None, load_limit: float = 0.35,
                 growth_step_log2: int = 2, prefetch_growth: bool = True, async_growth: bool = True,
                 verify_growth: bool = False, freeze_load: "float | None" = 0.5, symmetric: bool = False):
        self.device = _require_gpu(device)
        self._L = N.lib_for(self.device)
        self.symmetric = bool(symmetric)
        if self.symmetric and board_size != 4:
            raise ValueError("symmetric=True (Q2048_FLAG_SYMMETRIC) folds 4x4 boards only")
        self.on_gpu = self.device.type == "cuda"
        if action_space != 4:
            raise ValueError("the 2048 action space has 4 actions")
        if board_size not in (4, 5):
            raise NotImplementedError("board_size must be 4 (the reference) or 5")
        self.board_size, self.cells = int(board_size), int(board_size) ** 2
        self.growable = capacity_log2 == "auto"
        self.load_limit, self.growths = float(load_limit), []
        self.growth_step_log2, self.prefetch_growth = max(1, int(growth_step_log2)), bool(prefetch_growth)
        self.async_growth, self.verify_growth = bool(async_growth), bool(verify_growth)
        self._growth = self._retiring = None      # a growth being prepared / one committed and not yet finished
        if freeze_load is not None and not 0.05 <= float(freeze_load) <= 0.95:
            raise ValueError("freeze_load must be in [0.05, 0.95], or None (never freeze)")
        self.freeze_load = None if freeze_load is None else float(freeze_load)
        self.frozen, self.frozen_at = False, None  # the key set is closed (Q2048_FLAG_NO_NEW_ROWS on every launch)
        # a 4x4 table with a closed key set carries LINE SUMMARIES (q2048_table_summarise, Q2048_FLAG_LINE_SUMMARY): one
        # request per lookup of an absent state instead of 2.35 -- written by the first launch after the key set closed
        self.line_summaries, self._summarised = True, False
        # a 5x5 slot has no spare word: its summaries live BESIDE the table (q2048_table_summarise_side: 8 bytes per
        # 128-byte line, 1/16 of the table), allocated and written by the first learning launch after the key set
        # closed.  `_side`: the array while it describes this table's key set, else None (`side_summarised`);
        # `_side_refused`: the capacity whose array the device had no room for (slot by slot from then on)
        self._side, self._side_refused = None, None
        if self.growable:
            if not 0.05 <= self.load_limit <= 0.9:
                raise ValueError("load_limit must be in [0.05, 0.9]")
            if self.on_gpu:
                free, _ = torch.cuda.mem_get_info(self.device)
                share = free / _ranks_on_this_device()
            else:                                 # the CPU twin: host memory, a quarter of what is available
                share = 0.25 * os.sysconf("SC_AVPHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")
                self.async_growth = self.prefetch_growth = False    # (grows by export + import: `grow_table`)
                if initial_capacity_log2 == "auto":
                    initial_capacity_log2 = 22
            if initial_capacity_log2 == "auto":   # an eighth of the free memory, at most 2^30 slots (32 GiB)
                initial_capacity_log2 = min(30, max(20, int(np.floor(np.log2(max(share / 8 / N.SIZEOF_SLOT, 2.0))))))
            capacity_log2 = int(initial_capacity_log2)
            # the largest table that fits next to its predecessor while the rows move over -- and next to the retired
            # tables of earlier growths, which are kept until their memory is needed: with fourfold steps everything
            # below the largest table adds up to a third of it, the uneven last step to a little more (1.7 in all)
            fit = int(np.floor(np.log2(max(0.9 * share / (1.7 * N.SIZEOF_SLOT), 16.0))))
            self.max_capacity_log2 = max(capacity_log2, min(int(max_capacity_log2 or 34), fit, 40))
            placement = "chunks" if self.on_gpu else "plain"   # on a GPU growth is a property of the chunk allocator
        else:
            self.max_capacity_log2 = int(capacity_log2)
        if not self.on_gpu:
            placement = "plain"
        if not 4 <= capacity_log2 <= 40:
            raise ValueError("capacity_log2 must be in [4, 40]")
        self.action_space = action_space                                       # :21
        self.lr = learning_rate                                                # :17
        self.gamma = discount_factor                                           # :18
        self.schedule = EpsilonSchedule(total_epochs, exploration_rate, exploration_min)
        self.total_epochs = total_epochs
        self.capacity_log2 = int(capacity_log2)
        self.seed, self.env_id0 = int(seed), int(env_id0)
        self.flags = (N.FLAG_INDEPENDENT if independent else 0) | (N.FLAG_TD_CAS if strict_td else 0)
        # (Q2048_FLAG_SYMMETRIC is not in `flags`: only the entry points that take it get it, `_sym`)
        self._sym = N.FLAG_SYMMETRIC if self.symmetric else 0
        self.experiment_bits = 0  # unstable tuning bits OR-ed into fused_rollout's flags
        self.ctr = 0  # choose_action calls so far = counter word of the step draws
        try:
            self.table, self.placement = place_table(self.capacity_log2, self.device, placement,
                                                     self.max_capacity_log2 if self.growable else None)
        except (N.NativeError, RuntimeError) as exc:
            if not self.growable:
                raise
            # no virtual-memory API on this stack, or no room: one fixed table, as large as a quarter of the
            # free memory allows (at most 2^30 slots), from the ordinary allocator -- and say so
            self.growable = False
            self.capacity_log2 = self.max_capacity_log2 = auto_capacity_log2(0, self.device, floor_log2=30)
            warnings.warn(f'capacity_log2="auto": the growing table could not be mapped ({exc}); using a fixed '
                          f"table of 2^{self.capacity_log2} slots instead (updates beyond it are dropped and counted)")
            self.table, self.placement = place_table(self.capacity_log2, self.device, "plain")
            self.placement["growable_failed"] = str(exc)
        # row bookkeeping (growth, `verify_table`): the rows in the table are known EXACTLY at any stream point --
        # the rows counted at the last count / import (`_rows_base`) + the rows the kernels created since
        # (Q2048_ST_INSERTS, cumulative over statistics resets: `_inserts_folded`) -- at the price of one 8-byte
        # synchronising read, which `_room_for` pays only when an upper bound kept on the host (two new rows per
        # env-step launched since the last read) says a threshold may have been passed
        self._rows_base, self._inserts_at_base = 0, 0
        self._inserts_folded, self._inserts_seen, self._steps_unseen = 0, 0, 0
        self._steps_at_read, self._steps_launched, self._row_rate = 0, 0, 1.0
        self._warned_full = False
        self.stats_i, self.stats_f = new_stats_vectors(self.device)
        self._play_stats = None                   # the greedy player's own statistics (`play_rollout`), made when first used
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.q_table = _QTableView(self)
        self.row_cache_enabled = bool(row_cache)
        self._row_cache = None
        # statistics mirror of the fused rollout: the launch's last block copies both vectors into pinned
        # host memory the kernels address directly (q2048_rollout_opts.stats_mirror)
        self._mirror = _host_zeros(N.MIRROR_WORDS, torch.int64, self.device)
        self._mirror_np = self._mirror.numpy()
        self._mirror_ticket = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._mirror_launches = 0
        if self.growable and self.async_growth and self.prefetch_growth:
            self._begin_growth()                  # the next table is being mapped while the run sets itself up

    def _cache(self, B: int):
        """The row cache for a batch of B envs (device pointer or None)."""
        if not self.row_cache_enabled:
            return None
        c = self._row_cache
        if c is None or c.shape[0] != B:
            c = self._row_cache = torch.zeros((B, int(self._L.q2048_sizeof_rowcache(self.board_size))),
                                              dtype=torch.uint8, device=self.device)
        return c

    @property
    def side_summarised(self) -> bool:
        """A 5x5 table's line summaries (the array beside it) describe its key set as it is now."""
        return self._side is not None

    def _alloc_side_summaries(self, words: int) -> torch.Tensor:
        """The side array of a 5x5 table: `words` 8-byte words on the agent's device."""
        return torch.empty(words, dtype=torch.int64, device=self.device)

    def _side_summaries(self):
        """The line summaries of a 5x5 table whose key set is closed, for a learning launch of `fused_rollout`: the
        array beside the table, allocated (2^(capacity_log2-2) words) and written -- one streaming pass, queued ahead of
        the launch -- when there is none that describes this key set.  None when the launch has to probe slot by slot:
        `line_summaries` off, or the device had no room for the array (one warning, no further attempt)."""
        if not self.line_summaries or self._side_refused == self.capacity_log2:
            return None
        if self._side is None:
            try:
                side = self._alloc_side_summaries(1 << (self.capacity_log2 - 2))
            except (RuntimeError, MemoryError) as exc:    # (torch.OutOfMemoryError is a RuntimeError)
                self._side_refused = self.capacity_log2
                warnings.warn(f"no room for the line summaries of the 5x5 Q-table ({8 << (self.capacity_log2 - 2)} bytes "
                              f"beside 2^{self.capacity_log2} slots: {exc}); lookups go on slot by slot (same results)")
                return None
            N.check(self._L.q2048_table_summarise_side(_ptr(self.table), self.capacity_log2, 2, _ptr(side),
                                                       _stream(self.device)), "table_summarise_side")
            self._side = side
        return self._side

    def invalidate_row_cache(self) -> None:
        """After the table was changed by anything but choose_action / update_q_value."""
        if self._row_cache is not None:
            self._row_cache.zero_()

    # -- reference surface ---------------------------------------------------------------
    @property
    def epsilon(self) -> float:
        return self.schedule.epsilon

    @epsilon.setter
    def epsilon(self, v: float):
        self.schedule.epsilon = float(v)

    @property
    def epsilon_min(self) -> float:
        return self.schedule.epsilon_min

    def decay_exploration(self, current_epoch) -> None:
        self.schedule.decay_exploration(current_epoch)                         # :45-57

    def choose_action(self, boards: torch.Tensor) -> torch.Tensor:
        """choose_action (:34-38) for B states -> uint8 actions [B]."""
        self._refuse_symmetric("choose_action")
        boards = self._boards(boards)
        B = boards.shape[0]
        actions = torch.empty(B, dtype=torch.uint8, device=self.device)
        if B == 0:                               # (an empty batch: nothing to choose, and no draw is consumed)
            return actions
        N.check(self._L.q2048_q_choose_cached(
            _ptr(self.table), self.capacity_log2, _ptr(boards), B, self.board_size, float(self.epsilon),
            self.seed, self.env_id0, self.ctr & 0xFFFFFFFF, self._learn_flags(), _ptr(self._cache(B)), _ptr(actions),
            _ptr(self.status), _stream(self.device)), "q_choose")
        self.ctr += 1
        return actions

    def update_q_value(self, boards, actions, reward, next_boards, done) -> None:
        """update_q_value (:40-43) for B transitions."""
        self._refuse_symmetric("update_q_value")
        boards, next_boards = self._boards(boards), self._boards(next_boards)
        B = boards.shape[0]
        actions = self._vec(actions, torch.uint8, B, "actions")
        reward = self._vec(reward, torch.float32, B, "reward")
        done = self._vec(done, torch.uint8, B, "done")
        if B == 0:
            return
        self._room_for(B)
        N.check(self._L.q2048_q_update_cached(
            _ptr(self.table), self.capacity_log2, _ptr(boards), _ptr(actions), _ptr(reward),
            _ptr(next_boards), _ptr(done), B, self.board_size, float(self.lr), float(self.gamma), self.env_id0,
            self._learn_flags(), _ptr(self._cache(B)), _ptr(self.stats_i), _ptr(self.status), _stream(self.device)),
            "q_update")

    def q_values(self, boards: torch.Tensor, env_id: int | None = None,
                 return_found: bool = False):
        """q_table[state] for B states -> float32 [B, 4] (zeros where absent).  In independent
        mode board i is looked up in the rows of env `env_id0 + i`, or, when `env_id` is given,
        every board in the rows of that one env.  A symmetric agent looks up the row of the board's canonical
        image and returns it in the board's own frame (q[a] is the value of action a ON THIS BOARD)."""
        boards = self._boards(boards)
        B = boards.shape[0]
        q = torch.empty((B, 4), dtype=torch.float32, device=self.device)
        found = torch.empty(B, dtype=torch.uint8, device=self.device) if return_found else None
        if B == 0:                               # (an empty batch has no data pointers to hand over)
            return (q, found.bool()) if return_found else q
        flags = self.flags | self._sym | (N.FLAG_SINGLE_ENV if env_id is not None else 0)
        N.check(self._L.q2048_q_lookup(
            _ptr(self.table), self.capacity_log2, _ptr(boards), B, self.board_size,
            self.env_id0 if env_id is None else int(env_id), flags, _ptr(q), _ptr(found),
            _ptr(self.status), _stream(self.device)), "q_lookup")
        return (q, found.bool()) if return_found else q

    def canonicalize(self, boards: torch.Tensor):
        """q2048_canonicalize for B 4x4 boards -> (canonical images uint8 [B, 16], g uint8 [B]): the image a
        symmetric table is keyed by, and which of the eight it is (include/q2048.h, Q2048_FLAG_SYMMETRIC)."""
        if self.board_size != 4:
            raise ValueError("canonical images are defined for 4x4 boards")
        boards = self._boards(boards)
        B = boards.shape[0]
        out, g = torch.empty_like(boards), torch.empty(B, dtype=torch.uint8, device=self.device)
        if B:
            N.check(self._L.q2048_canonicalize(_ptr(boards), B, 4, _ptr(out), _ptr(g), _stream(self.device)),
                    "canonicalize")
        return out, g

    def _refuse_symmetric(self, what: str) -> None:
        if self.symmetric:
            raise ValueError(f"{what} does not take Q2048_FLAG_SYMMETRIC (symmetric=True): a folded table learns "
                             "through fused_rollout and is read through q_values / play_rollout")

    # -- throughput entry point ----------------------------------------------------------
    def fused_rollout(self, env: BatchedGame2048Env, steps: int, episode_log: "EpisodeLog | None" = None,
                      play_only: bool = False, learn: bool = True) -> None:
        """`steps` iterations of choose -> step -> update -> accumulate -> reset-on-done
        (Agent/main.py:91-101, :81) for every env in ONE launch.  Statistics accumulate in
        `stats_i` / `stats_f` on the device (read them with `stats()`); with `episode_log` every
        finished episode also leaves one record (the reference's CSV row, :103-105).  The env's
        profile flags travel with the call.  `play_only`: no learner -- the table is neither read
        nor written (every row reads as zeros); with epsilon = 1 that is uniformly random play.
        `learn=False`: evaluation -- actions come from the stored rows, nothing is created or written."""
        if env.device != self.device:
            raise ValueError("env and agent live on different devices")
        if (env.seed, env.env_id0) != (self.seed, self.env_id0):
            raise ValueError("env and agent must share seed and env_id0 (one draw stream per env)")
        if env.board_size != self.board_size:
            raise ValueError("env and agent have different board sizes")
        if env.ctr != self.ctr:
            raise ValueError(f"env.ctr={env.ctr} and agent.ctr={self.ctr} are out of step")
        log = episode_log
        if learn and not play_only:
            self._room_for(env.num_envs * int(steps))
        # the row every env carries goes from launch to launch (and to choose_action / update_q_value)
        # through the row cache; a learner-less launch touches neither the table nor the cache
        cache = None if play_only else self._cache(env.num_envs)
        flags, side = self.flags, None
        if learn and not play_only:
            flags = self._learn_flags()
            if self.frozen and self.board_size == 5:      # (4x4: in the slots, `_learn_flags`)
                side = self._side_summaries()
                flags |= N.FLAG_LINE_SUMMARY if side is not None else 0
        opts = N.RolloutOpts(
            log=_ptr(log.records) if log is not None else None, log_capacity=log.capacity if log is not None else 0,
            log_count=_ptr(log.count) if log is not None else None, row_cache=_ptr(cache),
            stats_mirror=self._mirror.data_ptr() if self.stats_i is not None and self.stats_f is not None else None,
            mirror_ticket=_ptr(self._mirror_ticket), line_summary=_ptr(side))
        N.check(self._L.q2048_fused_rollout_opts(
            _ptr(env.boards), _ptr(env.aux), _ptr(self.table), self.capacity_log2, env.num_envs,
            self.board_size, int(steps), float(self.epsilon), float(self.lr), float(self.gamma), self.seed,
            self.env_id0, self.ctr & 0xFFFFFFFF,
            flags | self._sym | self.experiment_bits | env.env_flags |
            (N.FLAG_PLAY_ONLY if play_only else 0) | (0 if learn else N.FLAG_NO_LEARN),
            _ptr(self.stats_i), _ptr(self.stats_f), _ptr(self.status), C.byref(opts), _stream(self.device)),
            "fused_rollout")
        if env.num_envs > 0 and int(steps) > 0:
            self._mirror_launches += 1
        env.ctr += int(steps)
        self.ctr += int(steps)

    def play_rollout(self, env: BatchedGame2048Env, steps: int, epsilon: float = 0.0) -> None:
        """The greedy player (q2048_play_rollout): `steps` steps of every env in ONE launch, each the first maximum
        of the state's stored row over the moves that CHANGE the board (with probability `epsilon` a uniformly drawn
        legal move instead), the env step, and on done the episode statistics and the reset -- what
        `evaluate.py --policy legal` measures, without its four library calls and twenty torch kernels per step.
        The table is only read: nothing is learnt, created or cached.  The player is a function of (table, env):
        seed, env_id0 and the step counter are the ENV's (an evaluation batch need not be in step with the
        agent), `env.ctr` advances, `agent.ctr`, the row cache and the growth / freeze bookkeeping are untouched.
        Statistics go to a buffer of the player's own (`play_stats`), never into the training statistics."""
        if env.device != self.device:
            raise ValueError("env and agent live on different devices")
        if env.board_size != self.board_size:
            raise ValueError("env and agent have different board sizes")
        if self._play_stats is None:
            self._play_stats = new_stats_vectors(self.device)
        si, sf = self._play_stats
        N.check(self._L.q2048_play_rollout(
            _ptr(env.boards), _ptr(env.aux), _ptr(self.table), self.capacity_log2, env.num_envs, self.board_size,
            int(steps), float(epsilon), env.seed, env.env_id0, env.ctr & 0xFFFFFFFF,
            (self.flags & N.FLAG_INDEPENDENT) | self._sym | env.env_flags, _ptr(si), _ptr(sf), _ptr(self.status),
            _stream(self.device)), "play_rollout")
        env.ctr += int(steps)

    def play_stats(self, reset: bool = False) -> dict:
        """Synchronising host copy of the player's statistics (the dict of `stats()`; inserts and drops are 0)."""
        if self._play_stats is None:
            self._play_stats = new_stats_vectors(self.device)
        out = stats_dict(*(v.cpu().numpy() for v in self._play_stats))   # (read before the reset: on "cpu" these are views)
        if reset:
            for v in self._play_stats:
                v.zero_()
        return out

    def mirrored_stats(self):
        """(stats_i, stats_f) as the last `fused_rollout` launch left them, read from the host-side
        mirror its last block wrote -- no device call, no copy: valid once the caller has waited for that
        launch (stream / event / device synchronize).  Raises if the mirror is not that launch's."""
        m = self._mirror_np
        if int(m[N.MIRROR_SEQ]) & 0xFFFFFFFF != self._mirror_launches & 0xFFFFFFFF:
            raise RuntimeError(f"statistics mirror holds launch {int(m[N.MIRROR_SEQ])}, expected "
                               f"{self._mirror_launches}: wait for the launch before reading it")
        return m[:N.NSTAT_I].copy(), m[N.NSTAT_I:N.NSTAT_I + N.NSTAT_F].view(np.float64).copy()

    def deterministic_rollout(self, env: BatchedGame2048Env, steps: int) -> None:
        """Reproducible shared-table training (q2048_det_rollout_cached): per step every env acts on the
        table as it is at the start of the step, the updates are sorted on the device by a hash of
        (state, action) and each group is applied update by update in env order.  The result is a
        function of the inputs alone and equals the reference agent (with float32 rows) fed the same
        transitions in env order -- bit for bit, at any B (tested at 1 048 576 boards).  Six launches
        per step, 7.2e9 env-steps/s at 1 Mi boards: `fused_rollout` is the fast path, this one is
        the yard-stick."""
        self._refuse_symmetric("deterministic_rollout")
        if env.device != self.device or env.board_size != self.board_size:
            raise ValueError("env and agent do not match")
        if (env.seed, env.env_id0, env.ctr) != (self.seed, self.env_id0, self.ctr):
            raise ValueError("env and agent must share seed, env_id0 and step counter")
        B, L = env.num_envs, self._L
        need = int(L.q2048_det_workspace_bytes(B, self.capacity_log2))
        if need < 0:
            N.check(need, "det_workspace_bytes")
        ws = getattr(self, "_det_ws", None)
        if ws is None or ws.numel() < need + 256:
            ws = self._det_ws = torch.empty(need + 256, dtype=torch.uint8, device=self.device)
        base = (ws.data_ptr() + 255) & ~255                       # the workspace is 256-byte aligned
        self._room_for(B * int(steps))
        # closed key set: the envs' visit rows live in the row cache from step to step (and come from / go on to
        # fused_rollout and update_q_value in it); otherwise this step neither reads nor keeps the records valid
        cache = self._cache(B) if self.frozen else None
        if cache is None:
            self.invalidate_row_cache()
        N.check(L.q2048_det_rollout_cached(
            _ptr(env.boards), _ptr(env.aux), _ptr(self.table), self.capacity_log2, B, self.board_size,
            int(steps), float(self.epsilon), float(self.lr), float(self.gamma), self.seed, self.env_id0,
            self.ctr & 0xFFFFFFFF, self._learn_flags() | env.env_flags | self.experiment_bits, _ptr(self.stats_i),
            _ptr(self.stats_f), _ptr(self.status), base, need, _ptr(cache), _stream(self.device)), "det_rollout")
        env.ctr += int(steps)
        self.ctr += int(steps)

    # -- a table that grows (capacity_log2="auto") ------------------------------------------------
    def _cumulative_inserts(self) -> int:
        return self._inserts_folded + int(self.stats_i[N.ST_INSERTS].item())

    def _rows_exact(self) -> int:
        """Rows in the table at this point of the stream: one synchronising 8-byte read of the kernels' own
        counter (no scan).  Also refreshes the rows-per-env-step estimate the growth policy plans with."""
        seen = self._cumulative_inserts()
        steps = self._steps_launched - self._steps_at_read
        if steps > 0:
            self._row_rate = min(2.0, max(0.02, 1.25 * (seen - self._inserts_seen) / steps))
        self._inserts_seen, self._steps_at_read, self._steps_unseen = seen, self._steps_launched, 0
        return self._rows_base + seen - self._inserts_at_base

    def _learn_flags(self) -> int:
        """The agent's flags for a call that may create rows: with the key set closed, Q2048_FLAG_NO_NEW_ROWS -- and,
        on a 4x4 table, Q2048_FLAG_LINE_SUMMARY once the summaries of THIS key set are written (one streaming pass,
        queued ahead of the first launch that uses them; a call that may create rows ends their validity).  A 5x5
        table's summaries lie beside it and only `fused_rollout` reads them (`_side_summaries`: pointer and flag are its
        business); what ends their validity is the same and is noted here."""
        if not self.frozen:
            self._summarised, self._side = False, None
            return self.flags
        if self.board_size == 4 and self.line_summaries and not self._summarised:
            N.check(self._L.q2048_table_summarise(_ptr(self.table), self.capacity_log2, _stream(self.device)),
                    "table_summarise")
            self._summarised = True
        return self.flags | N.FLAG_NO_NEW_ROWS | (N.FLAG_LINE_SUMMARY if self._summarised and self.line_summaries else 0)

    def _rebase_rows(self, rows: int, table_changed: bool = True) -> None:
        """`rows` rows are in the table now (a count, an import): the new base of the row bookkeeping."""
        if table_changed:
            self.frozen = False                           # (decided again by the next `_room_for`)
            self._summarised, self._side = False, None    # (line summaries describe a key set that is gone)
        self._rows_base = int(rows)
        self._inserts_at_base = self._inserts_seen = self._cumulative_inserts()
        self._steps_at_read, self._steps_unseen = self._steps_launched, 0

    def _room_for(self, env_steps: int) -> None:
        """Called before anything that may create rows: `env_steps` env-steps are about to be queued, each of
        which creates at most two rows (a state's own and its successor's, Agent/main.py:41-43).  Costs nothing
        while the host-side bound says no threshold can have been passed.  Otherwise the exact row count is read
        (8 bytes, synchronising) and
          - the next table starts being mapped (`prefetch_growth`: already at construction / after each growth;
            else when the rows expected after this call pass half the load limit),
          - the growth is committed -- the move queued between this launch and the previous one -- when the next
            table is ready AND the rows expected after this call (measured rows per env-step x 1.25) pass
            `load_limit` (a quarter of it when the table was prefetched: its memory is committed anyway, and the
            fewer rows there are the cheaper the move); while it is not ready the rollouts go on on the old table
            until the worst case (two rows per env-step) would pass load_limit + 0.25 (at most 0.85), and only
            then wait for it.
        A table that cannot grow (a fixed capacity, or the largest one) closes its key set at `freeze_load`
        (`_freeze_check`); with freeze_load=None it warns once when it passes the load limit."""
        env_steps = int(env_steps)
        self._steps_launched += env_steps
        if self.frozen:
            return
        if self._retiring is not None and self._retiring.ready():
            self._finish_retiring()
        if not self.growable or self.capacity_log2 >= self.max_capacity_log2:
            self._freeze_check(env_steps)
            return
        cap = 1 << self.capacity_log2
        soft, hard = self.load_limit * cap, min(0.85, self.load_limit + 0.25) * cap
        # the load at which this call has something to do: a prefetched table is moved into as soon as it is ready
        # and a quarter of the limit is in use (the fewer rows, the cheaper the move; the memory is committed
        # anyway); without prefetch the mapping begins at half the limit and the move waits for the limit
        commit_at = (0.25 if self.prefetch_growth else 1.0) * soft
        trigger = commit_at if self._growth is not None else min(0.5 * soft, commit_at)
        bound = self._rows_base + self._inserts_seen - self._inserts_at_base + 2 * (self._steps_unseen + env_steps)
        if bound <= trigger or (self._growth is not None and bound <= hard and not self._growth.ready()):
            self._steps_unseen += env_steps              # nothing to decide yet (or nothing to move into yet)
            return
        self._steps_launched -= env_steps                # (the read below must not count steps not yet queued)
        rows = self._rows_exact()
        self._steps_launched += env_steps
        self._steps_unseen = env_steps
        while True:
            cap = 1 << self.capacity_log2
            soft, hard = self.load_limit * cap, min(0.85, self.load_limit + 0.25) * cap
            commit_at = (0.25 if self.prefetch_growth else 1.0) * soft
            expect, worst = rows + self._row_rate * env_steps, rows + 2 * env_steps
            if self.capacity_log2 >= self.max_capacity_log2:   # (the last growth was just committed, or one failed)
                self._freeze_decide(rows)
                return
            if not self.async_growth:
                if expect > soft or worst > hard:
                    self.grow_table(min(self.capacity_log2 + self.growth_step_log2, self.max_capacity_log2), _rows=rows)
                    continue
                return
            if self._growth is None and (self.prefetch_growth or expect > 0.5 * soft):
                self._begin_growth()
            if self._growth is not None and (worst > hard or (expect > commit_at and self._growth.ready())):
                self._commit_growth(rows)
                continue                                  # (a launch larger than the new table's room: again)
            return

    def _freeze_check(self, env_steps: int) -> None:
        """A table that cannot grow, about to take `env_steps` more env-steps.  Free while the host-side bound (two
        new rows per env-step launched since the last read) stays below the threshold; else one synchronising 8-byte
        read of the kernels' insert counter and the decision (`_freeze_decide`)."""
        cap = 1 << self.capacity_log2
        limit = (self.freeze_load if self.freeze_load is not None else self.load_limit) * cap
        bound = self._rows_base + self._inserts_seen - self._inserts_at_base + 2 * (self._steps_unseen + env_steps)
        if bound <= limit or (self.freeze_load is None and self._warned_full):
            self._steps_unseen += env_steps
            return
        self._steps_launched -= env_steps                # (the read must not count steps not yet queued)
        rows = self._rows_exact()
        self._steps_launched += env_steps
        self._steps_unseen = env_steps
        self._freeze_decide(rows)

    def _freeze_decide(self, rows: int) -> None:
        """`rows` rows (exact, at this stream point) in a table that cannot grow: close the key set at freeze_load."""
        cap = 1 << self.capacity_log2
        if self.freeze_load is None:
            if rows > self.load_limit * cap and not self._warned_full:
                self._warned_full = True
                warnings.warn(f"the Q-table is at its largest capacity (2^{self.capacity_log2} slots) and holds "
                              f"{rows} rows (load {rows / cap:.2f} > {self.load_limit}) with freeze_load=None: lookups "
                              "slow down, and updates that find no slot within the probe limit are dropped and counted")
            return
        if rows < self.freeze_load * cap:
            return
        self.frozen = True
        self.frozen_at = {"rows": int(rows), "capacity_log2": self.capacity_log2, "load": rows / cap, "at_step": self.ctr}
        if not self._warned_full:
            self._warned_full = True
            warnings.warn(f"the Q-table cannot grow beyond 2^{self.capacity_log2} slots and holds {rows} rows (load "
                          f"{rows / cap:.2f} >= freeze_load {self.freeze_load}): it takes no new rows from here on -- rows "
                          "that exist keep learning, a state without a row reads as zeros (the defaultdict's fresh row) "
                          "and its updates are dropped and counted (stats()['drops'])")

    def _begin_growth(self) -> None:
        owner = getattr(self.table, "_q2048_owner", None)
        if owner is None or self.capacity_log2 >= self.max_capacity_log2:
            return
        new = min(self.capacity_log2 + self.growth_step_log2, self.max_capacity_log2)
        self._growth = owner.grow_begin(new)
        self._growth.info = {"begun_at_step": self.ctr}

    def _commit_growth(self, rows: int) -> None:
        """Queues the move of the `rows` rows (exact: read at this stream point) into the prepared table."""
        import time
        if self._retiring is not None:                    # the family's counters are free again after its check
            self._finish_retiring()
        g, t0 = self._growth, time.perf_counter()
        ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev[0].record()
        with torch.cuda.device(self.device):              # (raises with the old table intact and still self.table)
            try:
                bigger = g.commit(1 if self.board_size == 4 else 2, _stream(self.device), self.verify_growth)
            except N.NativeError as exc:
                self._growth = None
                if exc.code != N.ERR_ALLOC:
                    raise
                # the device has no room for the next table (other tenants, a smaller card): this capacity is the
                # largest from here on -- the run goes on, and `_room_for` warns when the load passes the limit
                self.max_capacity_log2 = self.capacity_log2
                warnings.warn(f"the Q-table cannot grow beyond 2^{self.capacity_log2} slots: the table of "
                              f"2^{g.new_capacity_log2} slots could not be mapped ({exc})")
                return
        ev[1].record()
        self.table = bigger.tensor(self.device)           # every launch from here on takes the new table
        self.table._q2048_owner = bigger
        g.info.setdefault("prepare_ms", round(g.wait(), 3))  # (ready by now: the commit has returned)
        g.info.update({"from_log2": self.capacity_log2, "to_log2": g.new_capacity_log2, "expected_rows": int(rows),
                       "at_step": self.ctr, "host_ms": round((time.perf_counter() - t0) * 1e3, 3), "events": ev})
        self.capacity_log2 = g.new_capacity_log2
        self.invalidate_row_cache()                       # slots changed
        self._side = None                                 # (and lines: another table, another size)
        self._growth, self._retiring = None, g
        if self.prefetch_growth:
            self._begin_growth()

    def _finish_retiring(self) -> None:
        """The committed growth's move is over (or is waited for): rows moved == rows the kernels created, else
        RuntimeError; the old table goes back to the device from the library's host thread."""
        g, self._retiring = self._retiring, None
        moved = g.finish()
        ev = g.info.pop("events")
        ev[1].synchronize()                               # (recorded right behind the library's own event)
        g.info.update({"rows": moved, "ms": round(ev[0].elapsed_time(ev[1]), 3)})
        self.growths.append(g.info)
        if moved != g.info["expected_rows"]:
            raise RuntimeError(f"Q-table self-check failed at the growth 2^{g.info['from_log2']} -> "
                               f"2^{g.info['to_log2']}: {moved} occupied slots moved, {g.info['expected_rows']} rows "
                               "created according to the kernels' counters")

    def wait_for_prefetch(self) -> "float | None":
        """Blocks until the table a prefetched growth is mapping is ready and returns what the library's host thread
        spent on it in ms (None: nothing is being prepared).  For a caller that wants the wait in its set-up rather
        than in its run: hipMemCreate of tens of GiB takes milliseconds on memory that has been free for a while and
        seconds when the driver is still wiping what a process released moments before."""
        if self._growth is None:
            return None
        ms = self._growth.wait()
        self._growth.info["prepare_ms"] = round(ms, 3)
        return ms

    def release_retired(self) -> None:
        """Gives the tables that earlier growths left behind back to the device now (q2048_table_trim): the library
        keeps them until their memory is needed, because freshly released memory makes the next mapping slow."""
        owner = getattr(self.table, "_q2048_owner", None)
        if owner is not None:
            self.finish_growth()
            N.check(self._L.q2048_table_trim(owner.ptr), "q2048_table_trim")

    def finish_growth(self) -> None:
        """Waits for a committed growth's move and runs its check (the end of a run, `verify_table`, tests)."""
        if self._retiring is not None:
            self._finish_retiring()

    def grow_table(self, new_capacity_log2: int | None = None, _rows: int | None = None) -> int:
        """Host-synchronous growth (q2048_table_grow): doubles the table (or takes it to 2**new_capacity_log2
        slots) -- the new capacity mapped onto fresh chunks in an address range of its own, every row moved over
        with one streaming kernel, the new table counted, the smaller one released.  Values are untouched, slots
        (and the table's address) change: the row cache is emptied.  30-180 ms up to 128 GiB on memory that has
        been free for a while.  Only tables made with capacity_log2="auto" can grow.  Returns the
        rows moved.  (`_room_for` uses the asynchronous begin / commit / finish form instead.)"""
        owner = getattr(self.table, "_q2048_owner", None)
        if not self.growable or (owner is None and self.on_gpu):
            raise RuntimeError('only a table made with capacity_log2="auto" can grow')
        new = self.capacity_log2 + 1 if new_capacity_log2 is None else int(new_capacity_log2)
        if not self.capacity_log2 < new <= self.max_capacity_log2:
            raise ValueError(f"cannot grow from 2^{self.capacity_log2} to 2^{new} slots "
                             f"(this table's largest capacity is 2^{self.max_capacity_log2})")
        if not self.on_gpu:
            return self._grow_on_host(new, _rows)
        self.finish_growth()
        if self._growth is not None:                      # a prepared table of another size: give it back
            g, self._growth = self._growth, None
            g.abort()
        expected = self._rows_exact() if _rows is None else int(_rows)
        t0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0[0].record()
        with torch.cuda.device(self.device):     # (raises with the old table intact and still self.table)
            bigger, moved = owner.grow(new, 1 if self.board_size == 4 else 2, _stream(self.device))
        self.table = bigger.tensor(self.device)  # the old tensor's memory is gone: nothing else may hold it
        self.table._q2048_owner = bigger
        t0[1].record()
        t0[1].synchronize()
        self.growths.append({"from_log2": self.capacity_log2, "to_log2": new, "rows": moved, "expected_rows": expected,
                             "ms": round(t0[0].elapsed_time(t0[1]), 3), "at_step": self.ctr})
        self.capacity_log2 = new
        self.invalidate_row_cache()
        self._side = None
        if moved != expected:
            raise RuntimeError(f"Q-table self-check failed at the growth to 2^{new}: {moved} occupied slots moved, "
                               f"{expected} rows created according to the kernels' counters")
        return moved

    def _grow_on_host(self, new: int, _rows: int | None) -> int:
        """The CPU twin's growth, through the ABI alone: every row exported, a larger table allocated, every row
        imported (host memory has no chunk allocator to ask; same check: rows moved == rows created)."""
        import time
        expected = self._rows_exact() if _rows is None else int(_rows)
        t0 = time.perf_counter()
        keys, q = self.export_rows()
        self.table = torch.zeros((1 << new, N.SIZEOF_SLOT), dtype=torch.uint8, device=self.device)
        old, self.capacity_log2 = self.capacity_log2, new
        self.invalidate_row_cache()
        self._side = None
        if len(q):
            tk = torch.from_numpy(np.ascontiguousarray(keys).view(np.int64).reshape(len(q), -1))
            self.import_rows_device(tk.reshape(-1) if self.board_size == 4 else tk, torch.from_numpy(q))
        if self.check_status() & N.STATUS_TABLE_FULL:
            raise RuntimeError("growth dropped rows (probe limit)")
        moved = self.table_size()
        self.growths.append({"from_log2": old, "to_log2": new, "rows": moved, "expected_rows": expected,
                             "ms": round((time.perf_counter() - t0) * 1e3, 3), "at_step": self.ctr})
        if moved != expected:
            raise RuntimeError(f"Q-table self-check failed at the growth to 2^{new}: {moved} rows moved, {expected} "
                               "rows created according to the counters")
        return moved

    def verify_table(self) -> dict:
        """Run-time check that no row was lost or duplicated: the slots occupied now == the rows counted
        at the last count / import + the rows the kernels say they created since (Q2048_ST_INSERTS).  One
        streaming pass over the table (1.3 ms per 8 GiB), synchronising -- for the end of a run, a checkpoint, a
        test; every growth runs the same check on the table it leaves behind without the extra pass.
        Raises RuntimeError on a mismatch; returns the numbers."""
        self.finish_growth()
        expect = self._rows_exact()
        rows = self.table_size()
        timeouts = N.claim_timeouts(self._L)
        if rows != expect or timeouts:
            raise RuntimeError(f"Q-table self-check failed: {rows} occupied slots, expected {expect} "
                               f"({self._rows_base} counted earlier + {expect - self._rows_base} created since); "
                               f"{timeouts} 5x5 claim time-outs")
        self._rebase_rows(rows, table_changed=False)
        return {"rows": rows, "capacity_log2": self.capacity_log2, "load": rows / float(1 << self.capacity_log2)}

    # -- statistics / table access ---------------------------------------------------------
    def stats(self, reset: bool = False, verify: bool = False) -> dict:
        """Synchronising host copy of the device statistics.  `verify`: also `verify_table()` -- the
        occupied slots must equal the rows counted earlier + the rows created since."""
        si = self.stats_i.cpu().numpy()
        sf = self.stats_f.cpu().numpy()
        if verify:
            self.verify_table()
        if reset:
            self._inserts_folded += int(si[N.ST_INSERTS])
            self.stats_i.zero_()
            self.stats_f.zero_()
        return stats_dict(si, sf)

    def table_size(self) -> int:
        """len(q_table): occupied slots."""
        count = torch.zeros(1, dtype=torch.int64, device=self.device)
        N.check(self._L.q2048_table_count(_ptr(self.table), self.capacity_log2, _ptr(count),
                                          _stream(self.device)), "table_count")
        return int(count.item())

    def export_rows(self):
        """All occupied rows on the host: (keys uint64 [R] for 4x4 / [R, 2] for 5x5,
        q float32 [R, 4])."""
        rows = self.table_size()
        words = 1 if self.board_size == 4 else 2
        keys = torch.empty((max(rows, 1), words), dtype=torch.int64, device=self.device)
        q = torch.empty((max(rows, 1), 4), dtype=torch.float32, device=self.device)
        count = torch.zeros(1, dtype=torch.int64, device=self.device)
        N.check(self._L.q2048_table_export(_ptr(self.table), self.capacity_log2, _ptr(keys),
                                           _ptr(q), rows, words, _ptr(count), _stream(self.device)),
                "table_export")
        got = min(int(count.item()), rows)
        k = keys[:got].cpu().numpy().view(np.uint64)
        return (k[:, 0] if words == 1 else k), q[:got].cpu().numpy()

    def export_dict(self, unfold: bool = False) -> dict:
        """The table in the reference's form: {tuple of 4 tuples of raw tile values ->
        np.float64[4]} (Agent/main.py:16,82).  Shared-table mode only.  A symmetric agent's table holds the
        CANONICAL states only -- one board per orbit of the eight symmetries, its row in that board's frame.
        unfold=True: a symmetric agent's table over ALL images instead, every board with the row `q_values` gives
        for it -- what the reference's loop needs, which knows nothing of canonical images; the table is unfolded on
        the device into a scratch plain agent (`unfold_from`) and that one is exported.  A plain agent's table is
        what it is either way."""
        if self.flags & N.FLAG_INDEPENDENT:
            raise ValueError("salted keys of independent mode do not decode to boards")
        if unfold and self.symmetric:
            self.finish_growth()
            room = max(4, int(np.ceil(np.log2(16.0 * max(self._rows_exact(), 1)))))   # eight images per row at load <= 0.5
            plain = BatchedQLearningAgent(1, capacity_log2=room, device=self.device, placement="plain", row_cache=False,
                                          freeze_load=None)
            plain.unfold_from(self)
            return plain.export_dict()
        keys, q = self.export_rows()
        out, n = {}, self.board_size
        for k, row in zip(keys.tolist(), q.astype(np.float64)):
            if n == 4:
                cells = [(k >> (4 * c)) & 15 for c in range(16)]
            else:  # 125 bits: key bits 0..62, then reserved bits 0..61
                big = (k[0] & ((1 << 63) - 1)) | ((k[1] & ((1 << 62) - 1)) << 63)
                cells = [(big >> (5 * c)) & 31 for c in range(25)]
            raw = [0 if v == 0 else 1 << v for v in cells]
            out[tuple(tuple(raw[n * r:n * r + n]) for r in range(n))] = row
        return out

    def check_status(self) -> int:
        s = int(self.status.item())
        if s & N.STATUS_BAD_ACTION:
            self.status.zero_()
            raise ValueError("an action outside 0..3 was passed to update_q_value()")
        return s

    # -- checkpoint / resume (the reference never saves its q_table) ------
    def state_dict(self, compact: bool = True) -> dict:
        """Host copy of the learner: the occupied rows (compact) or the raw table, the epsilon
        schedule, counters and statistics.  `load_state_dict` on an agent built with the same
        constructor arguments continues the run; compact rows are re-inserted, so slot positions
        may differ but every lookup returns the same values."""
        sd = {"capacity_log2": self.capacity_log2, "board_size": self.board_size,
              "flags": self.flags, "ctr": self.ctr, "seed": self.seed, "env_id0": self.env_id0,
              "lr": self.lr, "gamma": self.gamma, "schedule": dict(vars(self.schedule)),
              "stats_i": self.stats_i.to("cpu", copy=True), "stats_f": self.stats_f.to("cpu", copy=True)}
        if self.symmetric:
            sd["symmetric"] = True                # (a checkpoint without the field is a plain table)
        if compact:
            sd["keys"], sd["q"] = self.export_rows()
        else:
            sd["table"] = self.table.to("cpu", copy=True)
        if self.frozen and self._row_cache is not None:
            # closed key set: the envs' visit rows are part of the run (a resumed run equals the uninterrupted one
            # only with them); they live in the row cache, bound to this table's address (q2048_rowcache_rebind)
            sd["visit_rows"] = {"records": self._row_cache.to("cpu", copy=True), "table_address": int(self.table.data_ptr()),
                                "capacity_log2": self.capacity_log2}
        return sd

    def load_state_dict(self, sd: dict) -> None:
        if sd.get("kind") == "row_tuple":         # (a file without "kind" is a hash table: every earlier checkpoint)
            raise ValueError("this checkpoint holds row-tuple weights (BatchedRowTupleAgent), not a hash table: the "
                             "two kinds do not load into each other")
        if sd.get("kind") == "line_tuple":
            raise ValueError("this checkpoint holds line-tuple weights (BatchedLineTupleAgent), not a hash table: the "
                             "two kinds do not load into each other")
        if sd.get("kind") == "line_afterstate":
            raise ValueError("this checkpoint holds afterstate values (BatchedAfterstateAgent), not a hash table: the "
                             "two kinds do not load into each other")
        if sd.get("kind") == "ntuple6_afterstate":
            raise ValueError("this checkpoint holds a 6-tuple afterstate network (BatchedNTupleAgent), not a hash "
                             "table: the two kinds do not load into each other")
        if sd["board_size"] != self.board_size:
            raise ValueError("checkpoint was taken with another board size")
        if bool(sd.get("symmetric", False)) != self.symmetric:
            raise ValueError("a symmetry-folded table (symmetric=True) and a plain one do not load into each other: "
                             f"the checkpoint is {'folded' if sd.get('symmetric') else 'plain'}, this agent is "
                             f"{'folded' if self.symmetric else 'plain'}")
        self.ctr, self.seed, self.env_id0 = int(sd["ctr"]), int(sd["seed"]), int(sd["env_id0"])
        self.lr, self.gamma, self.flags = sd["lr"], sd["gamma"], int(sd["flags"])
        vars(self.schedule).update(sd["schedule"])
        self.stats_i.copy_(sd["stats_i"])
        self.stats_f.copy_(sd["stats_f"])
        self._inserts_folded = 0
        self.finish_growth()
        self.invalidate_row_cache()
        self.table.zero_()
        self._rebase_rows(0)                    # (the restored counters say nothing about this table yet)
        if "table" in sd:
            if sd["capacity_log2"] != self.capacity_log2:
                raise ValueError("raw tables only load into the same capacity")
            self.table.copy_(sd["table"])
        else:
            self.import_rows(sd["keys"], sd["q"])
        self._rebase_rows(self.table_size())
        v = sd.get("visit_rows")
        if v is not None and self.row_cache_enabled:
            # (the key set is the saved one; the launch that follows closes it again -- `_freeze_check` -- before it runs)
            rec = v["records"]
            self._row_cache = rec.to(self.device, copy=True).contiguous()
            N.check(self._L.q2048_rowcache_rebind(_ptr(self._row_cache), rec.shape[0], self.board_size, int(v["table_address"]),
                                                  int(v["capacity_log2"]), _ptr(self.table), self.capacity_log2,
                                                  _stream(self.device)), "rowcache_rebind")

    def import_rows(self, keys: np.ndarray, q: np.ndarray) -> None:
        """Inserts (key, q[4]) rows exported by `export_rows` (any capacity that holds them)."""
        rows = len(q)
        if rows == 0:                                   # (an empty table's checkpoint: nothing to reshape or insert)
            return
        keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(rows, -1)
        self.invalidate_row_cache()
        while self.growable and rows * 2 > (1 << self.capacity_log2) and self.capacity_log2 < self.max_capacity_log2:
            self.grow_table(min(self.max_capacity_log2,
                                max(self.capacity_log2 + 1, int(np.ceil(np.log2(2.0 * rows))))))
        # (a table that can grow is taken to load <= 0.5; one that cannot takes what a frozen table of its capacity
        # holds -- freeze_load plus a launch -- and the import's probe limit of 2^14 slots places rows up to load 0.93)
        if rows > 0.9 * (1 << self.capacity_log2):
            raise ValueError("table too small for the checkpoint (load factor would exceed 0.9)")
        tk = torch.from_numpy(keys.view(np.int64)).to(self.device)
        tq = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)   # this call's own word: the
        N.check(self._L.q2048_table_import(_ptr(self.table), self.capacity_log2, _ptr(tk), _ptr(tq),  # agent's
                                           rows, keys.shape[1], _ptr(status),                          # is sticky
                                           _stream(self.device)), "table_import")
        code = int(status.item())
        if code & N.STATUS_TABLE_FULL:
            raise RuntimeError("table_import dropped rows (probe limit)")
        if code & N.STATUS_DEEP_ROW:
            warnings.warn("table_import placed rows deeper than the learning paths probe (2^10 slots): q_values finds "
                          "them, choose / update / rollouts read them as absent -- load the checkpoint into a larger table")
        self._rebase_rows(self.table_size())

    def import_rows_device(self, keys: torch.Tensor, q: torch.Tensor) -> None:
        """q2048_table_import of rows that already live on the device: keys int64 [R] (4x4) or [R, 2] (5x5), q
        float32 [R, 4].  No growth, no count: the caller sizes the table and calls `recount_rows()` at the end
        (bulk loads, e.g. bench.py's pre-filled table)."""
        words = 1 if self.board_size == 4 else 2
        rows = int(q.shape[0])
        if keys.dtype != torch.int64 or q.dtype != torch.float32 or keys.numel() != rows * words or q.shape != (rows, 4):
            raise ValueError("keys must be int64 [R] / [R, 2] and q float32 [R, 4]")
        if rows == 0:
            return
        keys, q = keys.to(self.device).contiguous(), q.to(self.device).contiguous()
        self.invalidate_row_cache()
        self._summarised, self._side = False, None        # (rows arrive: line summaries stop describing the table)
        N.check(self._L.q2048_table_import(_ptr(self.table), self.capacity_log2, _ptr(keys), _ptr(q), rows, words,
                                           _ptr(self.status), _stream(self.device)), "table_import")

    _MERGE_MODES = {"add": N.MERGE_ADD, "blend": N.MERGE_BLEND, "maxabs": N.MERGE_MAXABS}

    def _combine_begin(self, other, what: str, kind_checks, mode: str, weight: float, rows_per_row: int, n_counters: int):
        """The common front of merge_from / fold_from / unfold_from (`what`: "merge", "fold", "unfold"): the checks of
        `other`, then the caller's own (`kind_checks()` raises), then mode, weight and the frozen rule; both growths
        finished; the table sized for rows + rows_per_row * other's rows, an upper bound of the rows afterwards; row
        cache and summaries invalidated.  Returns (rows, weight, counters, status): this agent's rows before the call,
        and the call's own zeroed counters and status word (the agent's status is sticky)."""
        if not isinstance(other, BatchedQLearningAgent) or other is self:
            raise ValueError(f"{what}_from takes another BatchedQLearningAgent")
        if other.device != self.device:
            raise ValueError("the two agents live on different devices")
        kind_checks()
        if mode not in self._MERGE_MODES:
            raise ValueError(f"mode must be one of {sorted(self._MERGE_MODES)}")
        weight = float(weight)
        if not np.isfinite(weight) or (mode == "blend" and not 0.0 <= weight <= 1.0):
            raise ValueError("weight must be finite, and in [0, 1] for mode 'blend'")
        if self.frozen:
            raise ValueError(f"this agent's key set is closed (frozen): {'an' if what[0] in 'aeiou' else 'a'} {what} "
                             "would create rows its visit rows and line summaries do not know")
        self.finish_growth()
        other.finish_growth()
        rows = self._rows_exact()
        total = rows + rows_per_row * other._rows_exact()
        while self.growable and total * 2 > (1 << self.capacity_log2) and self.capacity_log2 < self.max_capacity_log2:
            self.grow_table(min(self.max_capacity_log2, max(self.capacity_log2 + 1, int(np.ceil(np.log2(2.0 * total))))),
                            _rows=rows)
        if total > 0.9 * (1 << self.capacity_log2):
            raise ValueError(f"table too small for the {what} (load factor could exceed 0.9)")
        self.invalidate_row_cache()
        self._summarised, self._side = False, None        # (rows arrive: line summaries stop describing the table)
        return (rows, weight, torch.zeros(n_counters, dtype=torch.int64, device=self.device),
                torch.zeros(1, dtype=torch.int32, device=self.device))

    def _combine_end(self, what: str, unit: str, rows: int, counters, status, verify=None) -> list:
        """The common back: reads the call's counters ([..., created, combined, dropped]) and status, rebases the row
        bookkeeping (rows before + rows created), raises on TABLE_FULL, lets `verify(counts)` raise, warns on DEEP_ROW.
        Returns the counters as ints."""
        counts = [int(v) for v in counters.tolist()]
        created, dropped = counts[-3], counts[-1]
        code = int(status.item())
        self._rebase_rows(rows + created)
        if code & N.STATUS_TABLE_FULL:
            raise RuntimeError(f"table_{what} dropped {dropped} {unit} (probe limit)")
        if verify is not None:
            verify(counts)
        if code & N.STATUS_DEEP_ROW:
            warnings.warn(f"table_{what} placed rows deeper than the learning paths probe (2^10 slots): q_values finds "
                          f"them, choose / update / rollouts read them as absent -- {what} into a larger table")
        return counts

    def merge_from(self, other: "BatchedQLearningAgent", mode: str = "add", weight: float = 1.0) -> dict:
        """Combines `other`'s table into this one on the device (q2048_table_merge): every row of `other` finds or
        creates its row here -- the replicas of a job, or two checkpoints, become one table without a trip through
        the host.  `other` is only read.
          "add"     q = q + weight * q_other; a state without a row is the defaultdict's zero row (Agent/main.py:16).
                    weight 1: the sum; K merges with weight 1/K into an empty agent: the mean over K replicas.
          "blend"   a state both have: q = (1 - weight) * q + weight * q_other; a state only `other` has: its row as
                    it is.  weight in [0, 1]: 0 keeps this agent's rows and adds the missing ones, 1 takes `other`'s.
          "maxabs"  per action the value of larger magnitude (an untrained entry is exactly 0).
        float32 with every product and sum rounded on its own: a float32 numpy model gives the same bits.
        Sizing follows `import_rows`: a table that can grow grows first until both tables' rows fit half of it; one
        that cannot raises ValueError when they would pass load 0.9 (nothing is launched then).  A destination whose
        key set is closed (`frozen`) is refused: its visit rows and line summaries describe a key set the merge would
        change.  The row bookkeeping stays exact without a counting pass (rows before + rows created).
        Returns the call's counters: {"read", "created", "combined", "dropped"}; read == other's rows."""
        def kind_checks():
            if other.board_size != self.board_size:
                raise ValueError("the two agents have different board sizes")
            if other.symmetric != self.symmetric:
                raise ValueError("a symmetry-folded table (symmetric=True) and a plain one cannot be merged")

        # (rows + other's rows bounds the rows afterwards: keys may be shared)
        rows, weight, counters, status = self._combine_begin(other, "merge", kind_checks, mode, weight, 1, 4)
        N.check(self._L.q2048_table_merge(_ptr(self.table), self.capacity_log2, _ptr(other.table), other.capacity_log2,
                                          1 if self.board_size == 4 else 2, self._MERGE_MODES[mode], weight,
                                          _ptr(counters), _ptr(status), _stream(self.device)), "table_merge")
        read, created, combined, dropped = self._combine_end("merge", "rows", rows, counters, status)
        return {"read": read, "created": created, "combined": combined, "dropped": dropped}

    _FOLD_KINDS = {"mean": N.FOLD_MEAN, "mean_trained": N.FOLD_MEAN_TRAINED, "sum": N.FOLD_SUM, "maxabs": N.FOLD_MAXABS}

    def fold_from(self, other: "BatchedQLearningAgent", fold: str = "mean_trained", mode: str = "add",
                  weight: float = 1.0) -> dict:
        """Folds `other`'s PLAIN table into this symmetry-folded one on the device (q2048_table_fold): the rows `other`
        holds for a board's up to eight mirror images become one row in the canonical frame, and that row finds or
        creates its row here, combined with it by `mode` / `weight` as `merge_from` combines a row.  The way into a
        folded table for a learner that was trained plain.  `other` is only read.
          fold  "mean"          per action the mean over the images that have a row
                "mean_trained"  per action the mean over the images whose entry is not exactly 0: an image the run
                                never updated for that action does not dilute the ones it did (0 when there is none)
                "sum"           per action the sum over the images that have a row
                "maxabs"        per action the entry of largest magnitude
        float32, every product and sum rounded on its own, a fixed order of the images: a float32 numpy model gives the
        same bits, whatever the slots the rows lie in.  Sizing, the frozen rule and the row bookkeeping are
        `merge_from`'s (rows + other's rows is still an upper bound).  Keys salted per env (independent=True) cannot
        be told from boards and are refused.
        Returns the call's counters: {"read", "orbits", "created", "combined", "dropped"}; read == other's rows,
        orbits == created + combined + dropped."""
        def kind_checks():
            if self.board_size != 4 or other.board_size != 4:
                raise ValueError("symmetry folding is built for board size 4 only")
            if not self.symmetric:
                raise ValueError("fold_from needs a symmetry-folded destination (symmetric=True); merge_from combines "
                                 "two tables of one kind")
            if other.symmetric:
                raise ValueError("the source is already symmetry-folded: merge_from combines two folded tables")
            if (self.flags | other.flags) & N.FLAG_INDEPENDENT:
                raise ValueError("keys salted per env (independent=True, Q2048_FLAG_INDEPENDENT) do not decode to "
                                 "boards and cannot be folded")
            if fold not in self._FOLD_KINDS:
                raise ValueError(f"fold must be one of {sorted(self._FOLD_KINDS)}")

        # (rows + other's rows is an upper bound: an orbit has at least one row in `other`)
        rows, weight, counters, status = self._combine_begin(other, "fold", kind_checks, mode, weight, 1, 5)
        N.check(self._L.q2048_table_fold(_ptr(self.table), self.capacity_log2, _ptr(other.table), other.capacity_log2, 1,
                                         self._FOLD_KINDS[fold], self._MERGE_MODES[mode], weight, _ptr(counters),
                                         _ptr(status), _stream(self.device)), "table_fold")
        read, orbits, created, combined, dropped = self._combine_end("fold", "orbits", rows, counters, status)
        return {"read": read, "orbits": orbits, "created": created, "combined": combined, "dropped": dropped}

    def unfold_from(self, other: "BatchedQLearningAgent", mode: str = "add", weight: float = 1.0) -> dict:
        """Unfolds `other`'s SYMMETRY-FOLDED table into this plain one on the device (q2048_table_unfold), `fold_from`'s
        inverse: every row of `other` becomes one row per mirror image of its board -- 8, or 4, 2, 1 for boards that
        are their own mirror images -- each in that image's own frame, exactly what `other` answers when it is asked
        about that board, and each finds or creates its row here, combined with it by `mode` / `weight` as
        `merge_from` combines a row.  The way out of a folded table for everything that only understands plain ones
        (`choose_action`, `update_q_value`, `deterministic_rollout`, the reference's own loop over `export_dict`).
        `other` is only read.  float32, every product and sum rounded on its own: a float32 numpy model gives the
        same bits.  The frozen rule and the row bookkeeping are `merge_from`'s; sizing takes the upper bound
        rows + 8 * other's rows: a table that can grow grows first until that fits half of it, one that cannot
        raises ValueError when it would pass load 0.9 (nothing is launched then).
        Returns the call's counters: {"read", "skipped", "written", "created", "combined", "dropped"}; read == other's
        rows, written == created + combined + dropped.  skipped counts rows whose key is not canonical: a folded
        table never holds one, so anything but 0 raises RuntimeError (the table is corrupted)."""
        def kind_checks():
            if self.board_size != 4 or other.board_size != 4:
                raise ValueError("symmetry folding is built for board size 4 only")
            if self.symmetric:
                raise ValueError("unfold_from needs a plain destination (symmetric=False); merge_from combines two "
                                 "folded tables")
            if not other.symmetric:
                raise ValueError("the source is a plain table: merge_from combines two tables of one kind")
            if (self.flags | other.flags) & N.FLAG_INDEPENDENT:
                raise ValueError("keys salted per env (independent=True, Q2048_FLAG_INDEPENDENT) do not decode to "
                                 "boards and cannot be unfolded")

        def not_corrupted(counts):
            if counts[1]:
                raise RuntimeError(f"table_unfold skipped {counts[1]} rows of the folded table whose key is not "
                                   "canonical: the source table is corrupted")

        # (rows + 8 * other's rows is an upper bound: a row has at most eight images)
        rows, weight, counters, status = self._combine_begin(other, "unfold", kind_checks, mode, weight, 8, 6)
        N.check(self._L.q2048_table_unfold(_ptr(self.table), self.capacity_log2, _ptr(other.table), other.capacity_log2, 1,
                                           self._MERGE_MODES[mode], weight, _ptr(counters), _ptr(status),
                                           _stream(self.device)), "table_unfold")
        read, skipped, written, created, combined, dropped = self._combine_end("unfold", "rows", rows, counters, status,
                                                                               verify=not_corrupted)
        return {"read": read, "skipped": skipped, "written": written, "created": created, "combined": combined,
                "dropped": dropped}

    def recount_rows(self) -> int:
        """Counts the occupied slots (one streaming pass, synchronising) and makes that the base of the row
        bookkeeping: after anything but this class's own methods has written rows."""
        self.finish_growth()
        rows = self.table_size()
        self._rebase_rows(rows)
        return rows

    # -- argument plumbing -----------------------------------------------------------------
    def _boards(self, b) -> torch.Tensor:
        if not isinstance(b, torch.Tensor):
            b = torch.as_tensor(np.asarray(b, dtype=np.uint8))
        if b.dtype != torch.uint8:
            raise TypeError("boards must be uint8 log2 tiles")
        b = b.to(self.device)
        if b.dim() != 2 or b.shape[1] != self.cells:
            raise ValueError(f"boards must have shape (B, {self.cells}), got {tuple(b.shape)}")
        return b.contiguous()

    def _vec(self, v, dtype, B, name) -> torch.Tensor:
        if not isinstance(v, torch.Tensor):
            v = torch.as_tensor(v)
        if v.dtype == torch.bool and dtype == torch.uint8:
            v = v.view(torch.uint8)                     # same bytes: no copy, no kernel
        v = v.to(device=self.device, dtype=dtype).contiguous()
        if v.shape != (B,):
            raise ValueError(f"{name} must have shape ({B},), got {tuple(v.shape)}")
        return v


class BatchedRowTupleAgent:
    """BASELINE configs[1]: "flat-array Q over row-tuple features".  The reference's method names
    (choose_action / update_q_value / decay_exploration / epsilon) over a different table: a
    linear Q over the four 16-bit row indices, Q(s,a) = sum_r W[r][idx_r(s)][a], W float32
    [4, 65536, 4] (4 MiB).  It is NOT the reference's whole-board dict learner; it is
    validated against its own restatement in the oracle."""

    def __init__(self, total_epochs, action_space=4, learning_rate=0.1, discount_factor=0.9,
                 exploration_rate=1.0, exploration_min=0.01, device="cuda", seed: int = 0,
                 env_id0: int = 0):
        self.device = _require_gpu(device)
        self._L = N.lib_for(self.device)
        if action_space != 4:
            raise ValueError("the 2048 action space has 4 actions")
        self.lr, self.gamma = learning_rate, discount_factor
        self.schedule = EpsilonSchedule(total_epochs, exploration_rate, exploration_min)
        self.seed, self.env_id0, self.ctr, self.board_size = int(seed), int(env_id0), 0, 4
        self.weights = torch.zeros((4, 65536, 4), dtype=torch.float32, device=self.device)
        self.stats_i, self.stats_f = new_stats_vectors(self.device)
        self._play_stats = None                   # the player's own statistics (play_rollout / play_stats)
        self.status = torch.zeros(1, dtype=torch.int32, device=self.device)

    epsilon = property(lambda self: self.schedule.epsilon,
                       lambda self, v: setattr(self.schedule, "epsilon", float(v)))

    def decay_exploration(self, current_epoch) -> None:
        self.schedule.decay_exploration(current_epoch)

    def _boards(self, b) -> torch.Tensor:
        if not isinstance(b, torch.Tensor):
            b = torch.as_tensor(np.asarray(b, dtype=np.uint8))
        b = b.to(self.device)
        if b.dtype != torch.uint8 or b.dim() != 2 or b.shape[1] != 16:
            raise ValueError("boards must be uint8 with shape (B, 16)")
        return b.contiguous()

    def choose_action(self, boards) -> torch.Tensor:
        boards = self._boards(boards)
        B = boards.shape[0]
        actions = torch.empty(B, dtype=torch.uint8, device=self.device)
        N.check(self._L.q2048_rt_choose(_ptr(self.weights), _ptr(boards), B, float(self.epsilon),
                                        self.seed, self.env_id0, self.ctr & 0xFFFFFFFF, _ptr(actions),
                                        _stream(self.device)), "rt_choose")
        self.ctr += 1
        return actions

    def update_q_value(self, boards, actions, reward, next_boards, done) -> None:
        boards, next_boards = self._boards(boards), self._boards(next_boards)
        B = boards.shape[0]
        vec = lambda v, dt: torch.as_tensor(v).to(device=self.device, dtype=dt).contiguous()  # noqa: E731
        actions, reward, done = vec(actions, torch.uint8), vec(reward, torch.float32), vec(done, torch.uint8)
        if not (actions.shape == reward.shape == done.shape == (B,)):
            raise ValueError("actions / reward / done must have shape (B,)")
        N.check(self._L.q2048_rt_update(_ptr(self.weights), _ptr(boards), _ptr(actions), _ptr(reward),
                                        _ptr(next_boards), _ptr(done), B, float(self.lr),
                                        float(self.gamma), _ptr(self.status), _stream(self.device)),
                "rt_update")

    def q_values(self, boards) -> torch.Tensor:
        boards = self._boards(boards)
        q = torch.empty((boards.shape[0], 4), dtype=torch.float32, device=self.device)
        N.check(self._L.q2048_rt_lookup(_ptr(self.weights), _ptr(boards), boards.shape[0], _ptr(q),
                                        _stream(self.device)), "rt_lookup")
        return q

    def fused_rollout(self, env: BatchedGame2048Env, steps: int) -> None:
        if env.board_size != 4 or env.device != self.device:
            raise ValueError("the row-tuple learner needs a 4x4 env on the same device")
        if env.env_flags:
            raise ValueError("env profiles are supported by the hash-table agent only")
        if (env.seed, env.env_id0, env.ctr) != (self.seed, self.env_id0, self.ctr):
            raise ValueError("env and agent must share seed, env_id0 and step counter")
        N.check(self._L.q2048_rt_fused_rollout(
            _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), env.num_envs, int(steps),
            float(self.epsilon), float(self.lr), float(self.gamma), self.seed, self.env_id0,
            self.ctr & 0xFFFFFFFF, _ptr(self.stats_i), _ptr(self.stats_f), _ptr(self.status),
            _stream(self.device)), "rt_fused_rollout")
        env.ctr += int(steps)
        self.ctr += int(steps)

    def play_rollout(self, env: BatchedGame2048Env, steps: int, epsilon: float = 0.0) -> None:
        """The greedy player on the weights (q2048_rt_play_rollout), `BatchedQLearningAgent.play_rollout` with this
        learner's row: `steps` steps of every env in ONE launch, each the first maximum of `q_values(board)` over the
        moves that CHANGE the board (with probability `epsilon` a uniformly drawn legal move instead), the env step,
        and on done the episode statistics and the reset.  The weights are only read.  The player is a function of
        (weights, env): seed, env_id0 and the step counter are the ENV's, and so is its profile (`fused_rollout`
        keeps refusing profiles); `env.ctr` advances, `agent.ctr` does not.  Statistics go to a buffer of the
        player's own (`play_stats`), never into the training statistics."""
        if env.device != self.device:
            raise ValueError("env and agent live on different devices")
        if env.board_size != 4:
            raise ValueError("the row-tuple learner plays 4x4 boards only")
        if self._play_stats is None:
            self._play_stats = new_stats_vectors(self.device)
        si, sf = self._play_stats
        N.check(self._L.q2048_rt_play_rollout(
            _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), env.num_envs, int(steps), float(epsilon), env.seed,
            env.env_id0, env.ctr & 0xFFFFFFFF, env.env_flags, _ptr(si), _ptr(sf), _ptr(self.status),
            _stream(self.device)), "rt_play_rollout")
        env.ctr += int(steps)

    def play_stats(self, reset: bool = False) -> dict:
        """Synchronising host copy of the player's statistics (the dict of `stats()`; inserts and drops are 0)."""
        if self._play_stats is None:
            self._play_stats = new_stats_vectors(self.device)
        out = stats_dict(*(v.cpu().numpy() for v in self._play_stats))   # (read before the reset: on "cpu" these are views)
        if reset:
            for v in self._play_stats:
                v.zero_()
        return out

    def stats(self, reset: bool = False) -> dict:
        si, sf = self.stats_i.cpu().numpy(), self.stats_f.cpu().numpy()
        if reset:
            self.stats_i.zero_()
            self.stats_f.zero_()
        return stats_dict(si, sf)

    def check_status(self) -> int:
        s = int(self.status.item())
        if s & N.STATUS_BAD_ACTION:
            self.status.zero_()
            raise ValueError("an action outside 0..3 was passed to update_q_value()")
        return s

    # -- checkpoint / resume ------------------------------------------------------------------
    def state_dict(self, compact: bool = True) -> dict:
        """Host copy of the learner: {"kind": "row_tuple"}, the weights (float32 [4, 65536, 4]), lr / gamma, the
        epsilon schedule, seed / env_id0 / ctr and the two statistics vectors.  (`compact` is the hash-table
        agent's choice between rows and raw table; there is one form here.)"""
        return {"kind": "row_tuple", "board_size": 4, "weights": self.weights.to("cpu", copy=True), "lr": self.lr,
                "gamma": self.gamma, "schedule": dict(vars(self.schedule)), "seed": self.seed, "env_id0": self.env_id0,
                "ctr": self.ctr, "stats_i": self.stats_i.to("cpu", copy=True),
                "stats_f": self.stats_f.to("cpu", copy=True)}

    def load_state_dict(self, sd: dict) -> None:
        """Everything is validated before anything of this agent, on the host or the device, is written."""
        if sd.get("kind") != "row_tuple":
            raise ValueError("this checkpoint holds a hash table (BatchedQLearningAgent), not row-tuple weights: the "
                             "two kinds do not load into each other")
        if int(sd["board_size"]) != 4:
            raise ValueError("row-tuple weights are 4x4 only")
        w, si, sf = sd["weights"], sd["stats_i"], sd["stats_f"]
        if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or tuple(w.shape) != (4, 65536, 4):
            raise ValueError("weights must be a float32 tensor of shape (4, 65536, 4), got "
                             f"{getattr(w, 'dtype', type(w).__name__)} {tuple(getattr(w, 'shape', ()))}")
        if not isinstance(si, torch.Tensor) or si.dtype != torch.int64 or tuple(si.shape) != (N.NSTAT_I,) or \
                not isinstance(sf, torch.Tensor) or sf.dtype != torch.float64 or tuple(sf.shape) != (N.NSTAT_F,):
            raise ValueError(f"stats_i / stats_f must be int64 [{N.NSTAT_I}] / float64 [{N.NSTAT_F}]")
        schedule, ctr, seed, env_id0 = dict(sd["schedule"]), int(sd["ctr"]), int(sd["seed"]), int(sd["env_id0"])
        lr, gamma = float(sd["lr"]), float(sd["gamma"])
        self.weights.copy_(w)
        self.stats_i.copy_(si)
        self.stats_f.copy_(sf)
        self.ctr, self.seed, self.env_id0, self.lr, self.gamma = ctr, seed, env_id0, lr, gamma
        vars(self.schedule).update(schedule)


class BatchedLineTupleAgent(BatchedRowTupleAgent):
    """The row-tuple learner with the four COLUMNS as features beside the four rows (the "all lines" n-tuple layout):
    Q(s,a) = sum over the eight lines f of W[f][idx_f(s)][a], W float32 [8, 65536, 4] (8 MiB), features 0..3 the
    rows (the row-tuple indices), 4..7 the columns read from the top.  Same methods, checks, draws and TD target as
    `BatchedRowTupleAgent` (the error is spread over eight weights, lr / 8 each), through the q2048_lt_* entry
    points; a checkpoint says "kind": "line_tuple", and `load_row_tuple` promotes a row-tuple checkpoint."""

    N_FEATURES = 8

    def __init__(self, total_epochs, action_space=4, learning_rate=0.1, discount_factor=0.9,
                 exploration_rate=1.0, exploration_min=0.01, device="cuda", seed: int = 0,
                 env_id0: int = 0):
        super().__init__(total_epochs, action_space, learning_rate, discount_factor, exploration_rate,
                         exploration_min, device, seed, env_id0)
        self.weights = torch.zeros((self.N_FEATURES, 65536, 4), dtype=torch.float32, device=self.device)

    def choose_action(self, boards) -> torch.Tensor:
        boards = self._boards(boards)
        B = boards.shape[0]
        actions = torch.empty(B, dtype=torch.uint8, device=self.device)
        N.check(self._L.q2048_lt_choose(_ptr(self.weights), _ptr(boards), B, float(self.epsilon),
                                        self.seed, self.env_id0, self.ctr & 0xFFFFFFFF, _ptr(actions),
                                        _stream(self.device)), "lt_choose")
        self.ctr += 1
        return actions

    def update_q_value(self, boards, actions, reward, next_boards, done) -> None:
        boards, next_boards = self._boards(boards), self._boards(next_boards)
        B = boards.shape[0]
        vec = lambda v, dt: torch.as_tensor(v).to(device=self.device, dtype=dt).contiguous()  # noqa: E731
        actions, reward, done = vec(actions, torch.uint8), vec(reward, torch.float32), vec(done, torch.uint8)
        if not (actions.shape == reward.shape == done.shape == (B,)):
            raise ValueError("actions / reward / done must have shape (B,)")
        N.check(self._L.q2048_lt_update(_ptr(self.weights), _ptr(boards), _ptr(actions), _ptr(reward),
                                        _ptr(next_boards), _ptr(done), B, float(self.lr),
                                        float(self.gamma), _ptr(self.status), _stream(self.device)),
                "lt_update")

    def q_values(self, boards) -> torch.Tensor:
        boards = self._boards(boards)
        q = torch.empty((boards.shape[0], 4), dtype=torch.float32, device=self.device)
        N.check(self._L.q2048_lt_lookup(_ptr(self.weights), _ptr(boards), boards.shape[0], _ptr(q),
                                        _stream(self.device)), "lt_lookup")
        return q

    def fused_rollout(self, env: BatchedGame2048Env, steps: int) -> None:
        if env.board_size != 4 or env.device != self.device:
            raise ValueError("the line-tuple learner needs a 4x4 env on the same device")
        if env.env_flags:
            raise ValueError("env profiles are supported by the hash-table agent only")
        if (env.seed, env.env_id0, env.ctr) != (self.seed, self.env_id0, self.ctr):
            raise ValueError("env and agent must share seed, env_id0 and step counter")
        N.check(self._L.q2048_lt_fused_rollout(
            _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), env.num_envs, int(steps),
            float(self.epsilon), float(self.lr), float(self.gamma), self.seed, self.env_id0,
            self.ctr & 0xFFFFFFFF, _ptr(self.stats_i), _ptr(self.stats_f), _ptr(self.status),
            _stream(self.device)), "lt_fused_rollout")
        env.ctr += int(steps)
        self.ctr += int(steps)

    def play_rollout(self, env: BatchedGame2048Env, steps: int, epsilon: float = 0.0) -> None:
        """The greedy player on the weights (q2048_lt_play_rollout): `BatchedRowTupleAgent.play_rollout` with this
        learner's row.  The weights are only read; statistics go to `play_stats`."""
        if env.device != self.device:
            raise ValueError("env and agent live on different devices")
        if env.board_size != 4:
            raise ValueError("the line-tuple learner plays 4x4 boards only")
        if self._play_stats is None:
            self._play_stats = new_stats_vectors(self.device)
        si, sf = self._play_stats
        N.check(self._L.q2048_lt_play_rollout(
            _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), env.num_envs, int(steps), float(epsilon), env.seed,
            env.env_id0, env.ctr & 0xFFFFFFFF, env.env_flags, _ptr(si), _ptr(sf), _ptr(self.status),
            _stream(self.device)), "lt_play_rollout")
        env.ctr += int(steps)

    # -- checkpoint / resume / promotion ------------------------------------------------------
    def state_dict(self, compact: bool = True) -> dict:
        """`BatchedRowTupleAgent.state_dict` with "kind": "line_tuple" and weights float32 [8, 65536, 4]."""
        sd = super().state_dict(compact)
        sd["kind"] = "line_tuple"
        return sd

    @staticmethod
    def _validated(sd: dict, kind: str, features: int):
        """The fields of a row- or line-tuple checkpoint, all checked; nothing is written."""
        if sd.get("kind") != kind:
            held = {"row_tuple": "row-tuple weights (BatchedRowTupleAgent; `load_row_tuple` promotes them)",
                    "line_tuple": "line-tuple weights (BatchedLineTupleAgent)",
                    "line_afterstate": "afterstate values (BatchedAfterstateAgent)",
                    "ntuple6_afterstate": "a 6-tuple afterstate network (BatchedNTupleAgent)"}.get(
                        sd.get("kind"), "a hash table (BatchedQLearningAgent)")
            raise ValueError(f"this checkpoint holds {held}, not {kind.replace('_', '-')} weights: the kinds do not "
                             "load into each other")
        if int(sd["board_size"]) != 4:
            raise ValueError(f"{kind.replace('_', '-')} weights are 4x4 only")
        w, si, sf = sd["weights"], sd["stats_i"], sd["stats_f"]
        if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or tuple(w.shape) != (features, 65536, 4):
            raise ValueError(f"weights must be a float32 tensor of shape ({features}, 65536, 4), got "
                             f"{getattr(w, 'dtype', type(w).__name__)} {tuple(getattr(w, 'shape', ()))}")
        if not isinstance(si, torch.Tensor) or si.dtype != torch.int64 or tuple(si.shape) != (N.NSTAT_I,) or \
                not isinstance(sf, torch.Tensor) or sf.dtype != torch.float64 or tuple(sf.shape) != (N.NSTAT_F,):
            raise ValueError(f"stats_i / stats_f must be int64 [{N.NSTAT_I}] / float64 [{N.NSTAT_F}]")
        return (w, si, sf, dict(sd["schedule"]), int(sd["ctr"]), int(sd["seed"]), int(sd["env_id0"]),
                float(sd["lr"]), float(sd["gamma"]))

    def _take(self, si, sf, schedule, ctr, seed, env_id0, lr, gamma) -> None:
        self.stats_i.copy_(si)
        self.stats_f.copy_(sf)
        self.ctr, self.seed, self.env_id0, self.lr, self.gamma = ctr, seed, env_id0, lr, gamma
        vars(self.schedule).update(schedule)

    def load_state_dict(self, sd: dict) -> None:
        """Everything is validated before anything of this agent, on the host or the device, is written."""
        w, *rest = self._validated(sd, "line_tuple", self.N_FEATURES)
        self.weights.copy_(w)
        self._take(*rest)

    def load_row_tuple(self, sd: dict) -> None:
        """PROMOTION: takes a row-tuple checkpoint (`BatchedRowTupleAgent.state_dict`) -- its weights into features
        0..3, features 4..7 zeroed, and its schedule, counters and statistics.  `q_values` then equals the row-tuple
        agent's as values (the column half adds +0.0: only a -0.0 may change its sign bit), and the trained row
        weights go on learning with columns.  Validated before anything is written, like `load_state_dict`."""
        w, *rest = self._validated(sd, "row_tuple", 4)
        self.weights[:4].copy_(w)
        self.weights[4:].zero_()
        self._take(*rest)


class BatchedAfterstateAgent(BatchedLineTupleAgent):
    """The AFTERSTATE VALUE learner on the line features: V float32 [8, 65536] (2 MiB), one value per line entry.  A
    state is judged by the four boards its moves lead to before the spawn: q_a = merge score of move a + v(moved
    board), v = the sum of the moved board's eight entries; the choice is the player's in every method (greedy or
    exploring over the moves that change the board), and the TD step moves v(afterstate of the move played) towards
    gamma * (q of the greedy legal move of the next state), 0 at the end of a game.  The surface of
    `BatchedLineTupleAgent` through the q2048_av_* entry points; a checkpoint says "kind": "line_afterstate", and
    every other kind is refused in both directions -- Q entries are not afterstate values, so nothing is promoted."""

    def __init__(self, total_epochs, action_space=4, learning_rate=0.1, discount_factor=0.9,
                 exploration_rate=1.0, exploration_min=0.01, device="cuda", seed: int = 0,
                 env_id0: int = 0):
        super().__init__(total_epochs, action_space, learning_rate, discount_factor, exploration_rate,
                         exploration_min, device, seed, env_id0)
        self.weights = torch.zeros(self._SHAPE, dtype=torch.float32, device=self.device)

    # what tells this family from the one that inherits its surface (BatchedNTupleAgent): the entry points' prefix,
    # the weights' shape, the checkpoint's kind and the words of a refusal
    _FAMILY, _SHAPE, _KIND, _WHAT = "av", (8, 65536), "line_afterstate", "afterstate values"

    def _fn(self, name: str):
        return getattr(self._L, f"q2048_{self._FAMILY}_{name}")

    def choose_action(self, boards) -> torch.Tensor:
        boards = self._boards(boards)
        B = boards.shape[0]
        actions = torch.empty(B, dtype=torch.uint8, device=self.device)
        N.check(self._fn("choose")(_ptr(self.weights), _ptr(boards), B, float(self.epsilon),
                                        self.seed, self.env_id0, self.ctr & 0xFFFFFFFF, _ptr(actions),
                                        _stream(self.device)), self._FAMILY + "_choose")
        self.ctr += 1
        return actions

    def update_q_value(self, boards, actions, reward, next_boards, done) -> None:
        """The reference's signature; `reward` is IGNORED (only its shape is checked): the value of an afterstate
        estimates what comes after the move, and the learner's reward is the merge score of the next move, which
        the step reads off `next_boards`.  A lane whose action does not change its board writes nothing."""
        boards, next_boards = self._boards(boards), self._boards(next_boards)
        B = boards.shape[0]
        vec = lambda v, dt: torch.as_tensor(v).to(device=self.device, dtype=dt).contiguous()  # noqa: E731
        actions, done = vec(actions, torch.uint8), vec(done, torch.uint8)
        if not (actions.shape == tuple(torch.as_tensor(reward).shape) == done.shape == (B,)):
            raise ValueError("actions / reward / done must have shape (B,)")
        N.check(self._fn("update")(_ptr(self.weights), _ptr(boards), _ptr(actions), _ptr(next_boards),
                                        _ptr(done), B, float(self.lr), float(self.gamma), _ptr(self.status),
                                        _stream(self.device)), self._FAMILY + "_update")

    def q_values(self, boards) -> torch.Tensor:
        """q_a for the four actions (q2048_av_lookup): merge score + value of the moved board."""
        boards = self._boards(boards)
        q = torch.empty((boards.shape[0], 4), dtype=torch.float32, device=self.device)
        N.check(self._fn("lookup")(_ptr(self.weights), _ptr(boards), boards.shape[0], _ptr(q),
                                        _stream(self.device)), self._FAMILY + "_lookup")
        return q

    def values(self, boards) -> torch.Tensor:
        """v of each board as given (q2048_av_value)."""
        boards = self._boards(boards)
        v = torch.empty((boards.shape[0],), dtype=torch.float32, device=self.device)
        N.check(self._fn("value")(_ptr(self.weights), _ptr(boards), boards.shape[0], _ptr(v),
                                       _stream(self.device)), self._FAMILY + "_value")
        return v

    def fused_rollout(self, env: BatchedGame2048Env, steps: int) -> None:
        if env.board_size != 4 or env.device != self.device:
            raise ValueError("the afterstate learner needs a 4x4 env on the same device")
        if env.env_flags:
            raise ValueError("env profiles are supported by the hash-table agent only")
        if (env.seed, env.env_id0, env.ctr) != (self.seed, self.env_id0, self.ctr):
            raise ValueError("env and agent must share seed, env_id0 and step counter")
        N.check(self._fn("fused_rollout")(
            _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), env.num_envs, int(steps),
            float(self.epsilon), float(self.lr), float(self.gamma), self.seed, self.env_id0,
            self.ctr & 0xFFFFFFFF, _ptr(self.stats_i), _ptr(self.stats_f), _ptr(self.status),
            _stream(self.device)), self._FAMILY + "_fused_rollout")
        env.ctr += int(steps)
        self.ctr += int(steps)

    def play_rollout(self, env: BatchedGame2048Env, steps: int, epsilon: float = 0.0) -> None:
        """The greedy player on the values (q2048_av_play_rollout).  The weights are only read; statistics go to
        `play_stats`."""
        if env.device != self.device:
            raise ValueError("env and agent live on different devices")
        if env.board_size != 4:
            raise ValueError("the afterstate learner plays 4x4 boards only")
        if self._play_stats is None:
            self._play_stats = new_stats_vectors(self.device)
        si, sf = self._play_stats
        N.check(self._fn("play_rollout")(
            _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), env.num_envs, int(steps), float(epsilon), env.seed,
            env.env_id0, env.ctr & 0xFFFFFFFF, env.env_flags, _ptr(si), _ptr(sf), _ptr(self.status),
            _stream(self.device)), self._FAMILY + "_play_rollout")
        env.ctr += int(steps)

    @staticmethod
    def _search_depth(depth) -> int:
        if depth not in (1, 2) or isinstance(depth, bool):
            raise ValueError(f"search depth must be 1 or 2, not {depth!r}")
        return int(depth)

    def search_lookup(self, boards, depth: int = 1):
        """The SEARCHED row (q2048_av_search_lookup): one level of expectimax over the spawn.  For a legal move a,
        Q_a = merge score + the mean over the spawns of the moved board (a 2 with weight 9, a 4 with weight 1, in
        every empty cell) of the greedy value of the resulting state; 0.0 for a move that does not change the board.
        `depth=2` (q2048_av_search_lookup_depth) looks one level further: the value of a resulting state is the best
        of ITS searched row instead of its greedy value.
        Returns (q float32 [B, 4], legal uint8 [B]: bit a = move a changes the board)."""
        depth = self._search_depth(depth)
        boards = self._boards(boards)
        B = boards.shape[0]
        q = torch.empty((B, 4), dtype=torch.float32, device=self.device)
        legal = torch.empty((B,), dtype=torch.uint8, device=self.device)
        if depth == 1:
            N.check(self._fn("search_lookup")(_ptr(self.weights), _ptr(boards), B, _ptr(q), _ptr(legal),
                                              _stream(self.device)), self._FAMILY + "_search_lookup")
        else:
            N.check(self._fn("search_lookup_depth")(_ptr(self.weights), _ptr(boards), B, depth, _ptr(q), _ptr(legal),
                                                    _stream(self.device)), self._FAMILY + "_search_lookup_depth")
        return q, legal

    def search_rollout(self, env: BatchedGame2048Env, steps: int, epsilon: float = 0.0, depth: int = 1) -> None:
        """`play_rollout` with the searched row of `search_lookup` handed to the choice
        (q2048_av_search_play_rollout; `depth=2`: q2048_av_search_play_rollout_depth): same draws, env profiles,
        statistics (`play_stats`) and episode handling."""
        depth = self._search_depth(depth)
        if env.device != self.device:
            raise ValueError("env and agent live on different devices")
        if env.board_size != 4:
            raise ValueError("the afterstate learner plays 4x4 boards only")
        if self._play_stats is None:
            self._play_stats = new_stats_vectors(self.device)
        si, sf = self._play_stats
        if getattr(self, "stage_tiles", ()):      # the staged network (BatchedNTupleAgent): one entry point for both depths
            N.check(self._L.q2048_nts_search_play_rollout_depth(
                _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), self._stages, env.num_envs, int(steps), depth,
                float(epsilon), env.seed, env.env_id0, env.ctr & 0xFFFFFFFF, env.env_flags, _ptr(si), _ptr(sf),
                _ptr(self.status), _stream(self.device)), "nts_search_play_rollout_depth")
        elif depth == 1:
            N.check(self._fn("search_play_rollout")(
                _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), env.num_envs, int(steps), float(epsilon), env.seed,
                env.env_id0, env.ctr & 0xFFFFFFFF, env.env_flags, _ptr(si), _ptr(sf), _ptr(self.status),
                _stream(self.device)), self._FAMILY + "_search_play_rollout")
        else:
            N.check(self._fn("search_play_rollout_depth")(
                _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), env.num_envs, int(steps), depth, float(epsilon),
                env.seed, env.env_id0, env.ctr & 0xFFFFFFFF, env.env_flags, _ptr(si), _ptr(sf), _ptr(self.status),
                _stream(self.device)), self._FAMILY + "_search_play_rollout_depth")
        env.ctr += int(steps)

    def state_dict(self, compact: bool = True) -> dict:
        """`BatchedRowTupleAgent.state_dict` with "kind": "line_afterstate" and weights float32 [8, 65536]."""
        sd = BatchedRowTupleAgent.state_dict(self, compact)
        sd["kind"] = self._KIND
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Everything is validated before anything of this agent, on the host or the device, is written."""
        if sd.get("kind") != self._KIND:
            held = {"row_tuple": "row-tuple weights (BatchedRowTupleAgent)",
                    "line_tuple": "line-tuple weights (BatchedLineTupleAgent)",
                    "line_afterstate": "afterstate values (BatchedAfterstateAgent)",
                    "ntuple6_afterstate": "a 6-tuple afterstate network (BatchedNTupleAgent)"}.get(
                        sd.get("kind"), "a hash table (BatchedQLearningAgent)")
            raise ValueError(f"this checkpoint holds {held}, not {self._WHAT}: the kinds do not load into each "
                             "other (Q entries are not afterstate values, and the two afterstate families index "
                             "other features: nothing is promoted)")
        if int(sd["board_size"]) != 4:
            raise ValueError(f"{self._WHAT} are 4x4 only")
        w, si, sf = sd["weights"], sd["stats_i"], sd["stats_f"]
        if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or tuple(w.shape) != self._SHAPE:
            raise ValueError(f"weights must be a float32 tensor of shape {self._SHAPE}, got "
                             f"{getattr(w, 'dtype', type(w).__name__)} {tuple(getattr(w, 'shape', ()))}")
        if not isinstance(si, torch.Tensor) or si.dtype != torch.int64 or tuple(si.shape) != (N.NSTAT_I,) or \
                not isinstance(sf, torch.Tensor) or sf.dtype != torch.float64 or tuple(sf.shape) != (N.NSTAT_F,):
            raise ValueError(f"stats_i / stats_f must be int64 [{N.NSTAT_I}] / float64 [{N.NSTAT_F}]")
        rest = (si, sf, dict(sd["schedule"]), int(sd["ctr"]), int(sd["seed"]), int(sd["env_id0"]),
                float(sd["lr"]), float(sd["gamma"]))
        self.weights.copy_(w)
        self._take(*rest)

    def load_row_tuple(self, sd: dict) -> None:
        """Refused: a row- or line-tuple file holds Q entries per action, which are not afterstate values."""
        raise ValueError("Q entries are not afterstate values: a row-tuple or line-tuple checkpoint cannot be promoted "
                         f"into a {type(self).__name__}")


class BatchedNTupleAgent(BatchedAfterstateAgent):
    """The 6-TUPLE AFTERSTATE NETWORK with shared symmetric weights: V float32 [4, 16777216] (256 MiB).  Four 6-cell
    patterns, each read on the eight images of the board (the numbering of `symmetric=True`), one table per pattern
    shared by the eight images; v(board) = the sum of its 32 entries.  Everything else is `BatchedAfterstateAgent`
    -- q_a = merge score + v(moved board), the player's choice in every method, the TD step (the error spread over 32
    entries, lr / 32 each; a weight that a symmetric board reads several times moves once), `values`, the fused
    learner and the player -- through the q2048_nt_* entry points.  A checkpoint says "kind": "ntuple6_afterstate";
    every other kind is refused in both directions, and nothing is promoted.

    `coherence=True` gives every weight a step size of its own (temporal-coherence learning, q2048_nt_tc_*): the agent
    owns `self.coherence`, float32 [4, 16777216, 2] (512 MiB) of pairs {E, A} -- the signed sum of the weight's TD
    errors and the sum of their magnitudes -- and `update_q_value` / `fused_rollout` scale each entry's step by
    min(|E| / A, 1) (1 without history).  Everything that only reads V is inherited unchanged.  The checkpoint keeps
    its kind and carries the pairs under "coherence"; a plain agent loads such a file and ignores them, a coherence
    agent loads a plain file and starts its pairs at zero (rates restart at 1, same values).

    `stage_tiles=(2048,)` makes the network MULTI-STAGE (q2048_nts_*): one table per stage of the game, V float32
    [S, 4, 16777216] with S = 1 + the number of tiles given (powers of two, ascending, 2..32768, at most seven).  A
    board reads the table of the stage its largest tile has reached -- stage = the number of given tiles it is >= --
    and every candidate afterstate of an evaluation uses its own stage.  Every method goes through q2048_nts_*;
    `stage_tiles=()` is the plain agent on the plain entry points.  `promote()` copies what an earlier stage has
    learned into the entries of the next one that are still zero.  The checkpoint keeps its kind and carries
    "stage_tiles"; a staged agent loads a plain file into stage 0 and promotes it through every stage, a file with
    other tiles is refused, and a plain agent refuses a staged file.  Not combined with `coherence=True`.

    `carousel=P` (with `stage_tiles` only; 0 = off, and the agent is then the agent above) adds CAROUSEL SHAPING
    (q2048_car_*): `fused_rollout` starts episodes in turn at the beginning of every stage -- episode number e of a lane
    starts in stage e % S, from a board drawn from the agent's pool of boards on which earlier games entered that stage,
    or from an empty board where the pool has none -- and commits the boards its games recorded to the pool afterwards,
    on the same stream.  The agent owns `carousel_pool`, uint8 [S, P, 32], and `carousel_counts`, int64 [S] (records ever
    committed per stage), and allocates `carousel_fresh`, uint8 [S, B, 32], for the env's B at the first
    `fused_rollout`.  An "episode" of the statistics may then be a spliced game.  The four-call API, the players, the
    search and `promote()` are untouched.  The checkpoint keeps its kind and carries "carousel": {"pool", "counts"};
    a carousel agent loads a file without it (an empty pool), a plain staged agent ignores it, another P or S is
    refused.

    `trace_lambda=0.5` makes the learner TD(lambda) WITH A TRUNCATED TRACE (q2048_nt_lambda_*): the TD error of a step
    also moves the last `trace_depth` (0..3) afterstates the lane learned on in the current episode, the k-th of them by
    lambda^k of the step, and an explored move cuts the trace (Watkins).  `None` is the agent above on its own entry
    points.  The agent owns `self.trace`, int64 [B, 4] -- the count and three packed keys per lane -- allocated for the
    B of the first `fused_rollout` (or `update_q_value`); another B is refused.  `choose_action` goes through
    q2048_nt_choose_ex and keeps the flags as `last_explored`; `update_q_value(..., cut=None)` uses the flags of the
    `choose_action` before it.  The checkpoint keeps its kind and carries "trace": {"lambda", "depth", "keys"}; a plain
    agent ignores it, a trace agent loads a file without it and starts with empty traces, another B or depth is refused.
    Not combined with `coherence=True` or `stage_tiles`.

    `synchronous=True` makes the learner the SYNCHRONOUS BATCH STEP (q2048_nt_sync_*): in one step every lane evaluates
    against the same frozen weights, the TD errors that fall on a weight are summed exactly, as integers, and the weight
    moves once by their mean -- a pure function of its inputs at any batch size, the same bytes on the device and on
    "cpu" with any number of threads.  The agent owns `self.sync_acc`, int64 [4, 16777216, 2] (1 GiB), all zero between
    calls, and allocates `self.sync_pend`, int64 [B], for the B of the first `fused_rollout`; another B is refused, and
    B is at most 1,048,576.  Everything that only reads V is inherited, and the checkpoint is the plain agent's: plain
    and synchronous agents load each other's files.  Not combined with `coherence=True`, `stage_tiles`, `carousel` or
    `trace_lambda`."""

    _FAMILY, _SHAPE, _KIND, _WHAT = "nt", (4, 1 << 24), "ntuple6_afterstate", "a 6-tuple afterstate network"
    _ACC_SHAPE = (4, 1 << 24, 2)

    def __init__(self, total_epochs, action_space=4, learning_rate=0.1, discount_factor=0.9,
                 exploration_rate=1.0, exploration_min=0.01, device="cuda", seed: int = 0,
                 env_id0: int = 0, coherence: bool = False, stage_tiles=(), carousel: int = 0,
                 trace_lambda=None, trace_depth: int = 3, synchronous: bool = False):
        self.stage_tiles = self._check_stage_tiles(stage_tiles)
        if not isinstance(synchronous, bool):
            raise ValueError(f"synchronous must be True or False, not {synchronous!r}")
        if synchronous:
            for name, given in (("coherence=True", coherence), ("stage_tiles", self.stage_tiles),
                                ("carousel", carousel), ("trace_lambda", trace_lambda is not None)):
                if given:
                    raise ValueError(f"synchronous=True is not combined with {name}: q2048_nt_sync_* is the plain "
                                     "network's step")
        self.synchronous = synchronous
        self.sync_acc = self.sync_pend = None
        if trace_lambda is not None:
            if isinstance(trace_lambda, bool) or not isinstance(trace_lambda, (int, float)) \
                    or not 0.0 <= float(trace_lambda) <= 1.0:
                raise ValueError(f"trace_lambda must be a number in [0, 1] or None, not {trace_lambda!r}")
            if isinstance(trace_depth, bool) or not isinstance(trace_depth, int) or not 0 <= trace_depth <= 3:
                raise ValueError(f"trace_depth must be 0, 1, 2 or 3, not {trace_depth!r}")
            if coherence or self.stage_tiles:
                raise ValueError("trace_lambda is not combined with coherence=True or stage_tiles: q2048_nt_lambda_* "
                                 "knows one table and one step size")
        self.trace_lambda = None if trace_lambda is None else float(trace_lambda)
        self.trace_depth = int(trace_depth) if trace_lambda is not None else 0
        self.trace = self.last_explored = self._cut = None
        if isinstance(carousel, bool) or not isinstance(carousel, int) or carousel < 0 or carousel > 1 << 32:
            raise ValueError(f"carousel must be a number of records per stage from 0 (off) to 2^32, not {carousel!r}")
        if carousel and not self.stage_tiles:
            raise ValueError("carousel needs stage_tiles: the pool holds the boards on which games entered a stage")
        self.carousel = carousel
        if self.stage_tiles and coherence:
            raise ValueError("coherence=True is not combined with stage_tiles: q2048_nt_tc_* knows one table")
        # the stage spec of q2048_nts_*: nibble i = log2 of the (i + 1)-th threshold tile; 0 = the plain network
        self._stages = sum((t.bit_length() - 1) << (4 * i) for i, t in enumerate(self.stage_tiles))
        if self.stage_tiles:
            self._SHAPE = (len(self.stage_tiles) + 1,) + type(self)._SHAPE      # [S, 4, 2^24], allocated by the base
        super().__init__(total_epochs, action_space, learning_rate, discount_factor, exploration_rate,
                         exploration_min, device, seed, env_id0)
        self.coherence = torch.zeros(self._ACC_SHAPE, dtype=torch.float32, device=self.device) if coherence else None
        if self.synchronous:
            self.sync_acc = torch.zeros(self._ACC_SHAPE, dtype=torch.int64, device=self.device)
        self.carousel_pool = self.carousel_counts = self.carousel_fresh = None
        if self.carousel:
            S = len(self.stage_tiles) + 1
            self.carousel_pool = torch.zeros((S, self.carousel, 32), dtype=torch.uint8, device=self.device)
            self.carousel_counts = torch.zeros(S, dtype=torch.int64, device=self.device)

    @staticmethod
    def _check_stage_tiles(stage_tiles) -> tuple:
        tiles = tuple(stage_tiles)
        for t in tiles:
            if isinstance(t, bool) or not isinstance(t, int) or t < 2 or t > 32768 or t & (t - 1):
                raise ValueError(f"stage_tiles must be powers of two from 2 to 32768, not {t!r}")
        if any(a >= b for a, b in zip(tiles, tiles[1:])):
            raise ValueError(f"stage_tiles must ascend strictly, not {tiles!r}")
        if len(tiles) > 7:
            raise ValueError("at most seven stage_tiles (eight stages)")
        return tiles

    # ---- the staged network (stage_tiles given): every method through q2048_nts_*, the spec after the weights ----
    def _nts(self, name: str):
        return getattr(self._L, "q2048_nts_" + name)

    def _trace_for(self, B: int) -> torch.Tensor:
        if self.trace is None:
            self.trace = torch.zeros((B, 4), dtype=torch.int64, device=self.device)
        if self.trace.shape[0] != B:
            raise ValueError(f"this agent's traces are those of {self.trace.shape[0]} lanes, not of {B}")
        return self.trace

    def choose_action(self, boards) -> torch.Tensor:
        if self.trace_lambda is not None:
            boards = self._boards(boards)
            B = boards.shape[0]
            actions = torch.empty(B, dtype=torch.uint8, device=self.device)
            explored = torch.empty(B, dtype=torch.uint8, device=self.device)
            N.check(self._L.q2048_nt_choose_ex(_ptr(self.weights), _ptr(boards), B, float(self.epsilon), self.seed,
                                               self.env_id0, self.ctr & 0xFFFFFFFF, _ptr(actions), _ptr(explored),
                                               _stream(self.device)), "nt_choose_ex")
            self.ctr += 1
            self.last_explored = self._cut = explored
            return actions
        if not self.stage_tiles:
            return super().choose_action(boards)
        boards = self._boards(boards)
        B = boards.shape[0]
        actions = torch.empty(B, dtype=torch.uint8, device=self.device)
        N.check(self._nts("choose")(_ptr(self.weights), self._stages, _ptr(boards), B, float(self.epsilon),
                                    self.seed, self.env_id0, self.ctr & 0xFFFFFFFF, _ptr(actions),
                                    _stream(self.device)), "nts_choose")
        self.ctr += 1
        return actions

    def q_values(self, boards) -> torch.Tensor:
        if not self.stage_tiles:
            return super().q_values(boards)
        boards = self._boards(boards)
        q = torch.empty((boards.shape[0], 4), dtype=torch.float32, device=self.device)
        N.check(self._nts("lookup")(_ptr(self.weights), self._stages, _ptr(boards), boards.shape[0], _ptr(q),
                                    _stream(self.device)), "nts_lookup")
        return q

    def values(self, boards) -> torch.Tensor:
        if not self.stage_tiles:
            return super().values(boards)
        boards = self._boards(boards)
        v = torch.empty((boards.shape[0],), dtype=torch.float32, device=self.device)
        N.check(self._nts("value")(_ptr(self.weights), self._stages, _ptr(boards), boards.shape[0], _ptr(v),
                                   _stream(self.device)), "nts_value")
        return v

    def play_rollout(self, env: BatchedGame2048Env, steps: int, epsilon: float = 0.0) -> None:
        if not self.stage_tiles:
            return super().play_rollout(env, steps, epsilon)
        if env.device != self.device:
            raise ValueError("env and agent live on different devices")
        if env.board_size != 4:
            raise ValueError("the afterstate learner plays 4x4 boards only")
        if self._play_stats is None:
            self._play_stats = new_stats_vectors(self.device)
        si, sf = self._play_stats
        N.check(self._nts("play_rollout")(
            _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), self._stages, env.num_envs, int(steps), float(epsilon),
            env.seed, env.env_id0, env.ctr & 0xFFFFFFFF, env.env_flags, _ptr(si), _ptr(sf), _ptr(self.status),
            _stream(self.device)), "nts_play_rollout")
        env.ctr += int(steps)

    def search_lookup(self, boards, depth: int = 1):
        if not self.stage_tiles:
            return super().search_lookup(boards, depth)
        depth = self._search_depth(depth)
        boards = self._boards(boards)
        B = boards.shape[0]
        q = torch.empty((B, 4), dtype=torch.float32, device=self.device)
        legal = torch.empty((B,), dtype=torch.uint8, device=self.device)
        N.check(self._nts("search_lookup_depth")(_ptr(self.weights), self._stages, _ptr(boards), B, depth, _ptr(q),
                                                 _ptr(legal), _stream(self.device)), "nts_search_lookup_depth")
        return q, legal

    def promote(self) -> list:
        """BULK PROMOTION (q2048_nts_promote) over the pairs (0, 1), (1, 2), ... in ascending order: an entry of the
        later stage whose bits are all zero takes the bits of the earlier stage's entry, where those are not zero.
        Returns the number of entries copied per pair; synchronises."""
        if not self.stage_tiles:
            raise ValueError("this agent was built without stage_tiles")
        counts = torch.zeros(len(self.stage_tiles), dtype=torch.int64, device=self.device)
        for k in range(len(self.stage_tiles)):
            N.check(self._nts("promote")(_ptr(self.weights), self._stages, k, k + 1, _ptr(counts[k:]),
                                         _stream(self.device)), "nts_promote")
        return [int(c) for c in counts.tolist()]

    def update_q_value(self, boards, actions, reward, next_boards, done, cut=None) -> None:
        if self.trace_lambda is None and cut is not None:
            raise ValueError("cut is the trace learner's argument: this agent was built without trace_lambda")
        if self.synchronous:
            boards, next_boards = self._boards(boards), self._boards(next_boards)
            B = boards.shape[0]
            vec = lambda v, dt: torch.as_tensor(v).to(device=self.device, dtype=dt).contiguous()  # noqa: E731
            actions, done = vec(actions, torch.uint8), vec(done, torch.uint8)
            if not (actions.shape == tuple(torch.as_tensor(reward).shape) == done.shape == (B,)):
                raise ValueError("actions / reward / done must have shape (B,)")
            N.check(self._L.q2048_nt_sync_update(_ptr(self.weights), _ptr(self.sync_acc), _ptr(boards), _ptr(actions),
                                                 _ptr(next_boards), _ptr(done), B, float(self.lr), float(self.gamma),
                                                 _ptr(self.status), _stream(self.device)), "nt_sync_update")
            return None
        if self.trace_lambda is not None:
            boards, next_boards = self._boards(boards), self._boards(next_boards)
            B = boards.shape[0]
            vec = lambda v, dt: torch.as_tensor(v).to(device=self.device, dtype=dt).contiguous()  # noqa: E731
            actions, done = vec(actions, torch.uint8), vec(done, torch.uint8)
            if not (actions.shape == tuple(torch.as_tensor(reward).shape) == done.shape == (B,)):
                raise ValueError("actions / reward / done must have shape (B,)")
            if cut is None:
                if self._cut is None or self._cut.shape[0] != B:
                    raise ValueError("no choose_action of this batch size since the last update: pass cut=")
                cut = self._cut
            cut = vec(cut, torch.uint8)
            if cut.shape != (B,):
                raise ValueError("cut must have shape (B,)")
            trace = self._trace_for(B) if self.trace_depth else None
            N.check(self._L.q2048_nt_lambda_update(
                _ptr(self.weights), _ptr(trace) if trace is not None else None, _ptr(boards), _ptr(actions),
                _ptr(next_boards), _ptr(done), _ptr(cut), B, float(self.lr), float(self.gamma), self.trace_lambda,
                self.trace_depth, _ptr(self.status), _stream(self.device)), "nt_lambda_update")
            self._cut = None
            return None
        if self.stage_tiles:
            boards, next_boards = self._boards(boards), self._boards(next_boards)
            B = boards.shape[0]
            vec = lambda v, dt: torch.as_tensor(v).to(device=self.device, dtype=dt).contiguous()  # noqa: E731
            actions, done = vec(actions, torch.uint8), vec(done, torch.uint8)
            if not (actions.shape == tuple(torch.as_tensor(reward).shape) == done.shape == (B,)):
                raise ValueError("actions / reward / done must have shape (B,)")
            N.check(self._nts("update")(_ptr(self.weights), self._stages, _ptr(boards), _ptr(actions),
                                        _ptr(next_boards), _ptr(done), B, float(self.lr), float(self.gamma),
                                        _ptr(self.status), _stream(self.device)), "nts_update")
            return None
        if self.coherence is None:
            return super().update_q_value(boards, actions, reward, next_boards, done)
        boards, next_boards = self._boards(boards), self._boards(next_boards)
        B = boards.shape[0]
        vec = lambda v, dt: torch.as_tensor(v).to(device=self.device, dtype=dt).contiguous()  # noqa: E731
        actions, done = vec(actions, torch.uint8), vec(done, torch.uint8)
        if not (actions.shape == tuple(torch.as_tensor(reward).shape) == done.shape == (B,)):
            raise ValueError("actions / reward / done must have shape (B,)")
        N.check(self._L.q2048_nt_tc_update(_ptr(self.weights), _ptr(self.coherence), _ptr(boards), _ptr(actions),
                                           _ptr(next_boards), _ptr(done), B, float(self.lr), float(self.gamma),
                                           _ptr(self.status), _stream(self.device)), "nt_tc_update")

    def fused_rollout(self, env: BatchedGame2048Env, steps: int) -> None:
        if self.coherence is None and not self.stage_tiles and self.trace_lambda is None and not self.synchronous:
            return super().fused_rollout(env, steps)
        if env.board_size != 4 or env.device != self.device:
            raise ValueError("the afterstate learner needs a 4x4 env on the same device")
        if env.env_flags:
            raise ValueError("env profiles are supported by the hash-table agent only")
        if (env.seed, env.env_id0, env.ctr) != (self.seed, self.env_id0, self.ctr):
            raise ValueError("env and agent must share seed, env_id0 and step counter")
        if self.synchronous:
            if self.sync_pend is None:
                self.sync_pend = torch.zeros(env.num_envs, dtype=torch.int64, device=self.device)
            if self.sync_pend.shape[0] != env.num_envs:
                raise ValueError(f"this agent's step scratch is that of {self.sync_pend.shape[0]} lanes, not of "
                                 f"{env.num_envs}")
            N.check(self._L.q2048_nt_sync_fused_rollout(
                _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), _ptr(self.sync_acc), _ptr(self.sync_pend),
                env.num_envs, int(steps), float(self.epsilon), float(self.lr), float(self.gamma), self.seed,
                self.env_id0, self.ctr & 0xFFFFFFFF, _ptr(self.stats_i), _ptr(self.stats_f), _ptr(self.status),
                _stream(self.device)), "nt_sync_fused_rollout")
            env.ctr += int(steps)
            self.ctr += int(steps)
            return None
        if self.trace_lambda is not None:
            trace = self._trace_for(env.num_envs) if self.trace_depth else None
            N.check(self._L.q2048_nt_lambda_fused_rollout(
                _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), _ptr(trace) if trace is not None else None,
                env.num_envs, int(steps), float(self.epsilon), float(self.lr), float(self.gamma), self.trace_lambda,
                self.trace_depth, self.seed, self.env_id0, self.ctr & 0xFFFFFFFF, _ptr(self.stats_i),
                _ptr(self.stats_f), _ptr(self.status), _stream(self.device)), "nt_lambda_fused_rollout")
            env.ctr += int(steps)
            self.ctr += int(steps)
            return None
        if self.carousel:
            B, S = env.num_envs, len(self.stage_tiles) + 1
            if self.carousel_fresh is None or self.carousel_fresh.shape[1] != B:
                self.carousel_fresh = torch.zeros((S, B, 32), dtype=torch.uint8, device=self.device)
            N.check(self._L.q2048_car_fused_rollout(
                _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), self._stages, _ptr(self.carousel_pool),
                _ptr(self.carousel_counts), _ptr(self.carousel_fresh), self.carousel, B, int(steps),
                float(self.epsilon), float(self.lr), float(self.gamma), self.seed, self.env_id0,
                self.ctr & 0xFFFFFFFF, _ptr(self.stats_i), _ptr(self.stats_f), _ptr(self.status),
                _stream(self.device)), "car_fused_rollout")
            N.check(self._L.q2048_car_commit(_ptr(self.carousel_pool), _ptr(self.carousel_counts),
                                             _ptr(self.carousel_fresh), self._stages, self.carousel, B,
                                             _stream(self.device)), "car_commit")
            env.ctr += int(steps)
            self.ctr += int(steps)
            return None
        if self.stage_tiles:
            N.check(self._nts("fused_rollout")(
                _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), self._stages, env.num_envs, int(steps),
                float(self.epsilon), float(self.lr), float(self.gamma), self.seed, self.env_id0,
                self.ctr & 0xFFFFFFFF, _ptr(self.stats_i), _ptr(self.stats_f), _ptr(self.status),
                _stream(self.device)), "nts_fused_rollout")
            env.ctr += int(steps)
            self.ctr += int(steps)
            return None
        N.check(self._L.q2048_nt_tc_fused_rollout(
            _ptr(env.boards), _ptr(env.aux), _ptr(self.weights), _ptr(self.coherence), env.num_envs, int(steps),
            float(self.epsilon), float(self.lr), float(self.gamma), self.seed, self.env_id0,
            self.ctr & 0xFFFFFFFF, _ptr(self.stats_i), _ptr(self.stats_f), _ptr(self.status),
            _stream(self.device)), "nt_tc_fused_rollout")
        env.ctr += int(steps)
        self.ctr += int(steps)

    def carousel_summary(self) -> dict:
        """{"counts": records ever committed per stage, "valid": records a restart can draw per stage (min(count, P))};
        stage 0 has none by construction.  Synchronises."""
        if not self.carousel:
            raise ValueError("this agent was built without carousel=P")
        counts = [int(c) for c in self.carousel_counts.cpu().tolist()]
        return {"counts": counts, "valid": [min(c, self.carousel) for c in counts]}

    def coherence_summary(self) -> dict:
        """{"visited": the share of pairs with A > 0, "mean_rate": the mean of min(|E| / A, 1) over them (1.0 where
        there is none)}, by reductions on the agent's device; synchronises."""
        if self.coherence is None:
            raise ValueError("this agent was built without coherence=True")
        E, A = self.coherence[..., 0], self.coherence[..., 1]
        seen = A > 0
        n = int(seen.sum().item())
        rate = torch.where(seen, torch.clamp(E.abs() / A, max=1.0), torch.zeros((), device=self.device))
        total = float(rate.sum(dtype=torch.float64).item())
        return {"visited": n / seen.numel(), "mean_rate": total / n if n else 1.0}

    def state_dict(self, compact: bool = True) -> dict:
        """`BatchedAfterstateAgent.state_dict` ("kind": "ntuple6_afterstate", weights float32 [4, 16777216]); with
        `coherence=True` also "coherence", the pairs float32 [4, 16777216, 2]."""
        sd = super().state_dict(compact)
        if self.coherence is not None:
            sd["coherence"] = self.coherence.to("cpu", copy=True)
        if self.stage_tiles:
            sd["stage_tiles"] = list(self.stage_tiles)     # weights float32 [S, 4, 16777216]
        if self.carousel:
            sd["carousel"] = {"pool": self.carousel_pool.to("cpu", copy=True),
                              "counts": self.carousel_counts.to("cpu", copy=True)}
        if self.trace_lambda is not None:
            keys = self.trace.to("cpu", copy=True) if self.trace is not None else torch.zeros((0, 4), dtype=torch.int64)
            sd["trace"] = {"lambda": self.trace_lambda, "depth": self.trace_depth, "keys": keys}
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Everything -- the pairs included, where this agent takes them -- is validated before anything of this agent
        is written.  A plain agent ignores a file's pairs; a coherence agent without pairs in the file zeroes its own."""
        file_tiles = tuple(sd.get("stage_tiles") or ())
        tr = sd.get("trace") if self.trace_lambda is not None else None      # a plain agent ignores a file's traces
        if tr is not None:
            keys = tr.get("keys") if isinstance(tr, dict) else None
            if not isinstance(keys, torch.Tensor) or keys.dtype != torch.int64 or keys.dim() != 2 or keys.shape[1] != 4:
                raise ValueError("trace keys must be an int64 tensor of shape (B, 4)")
            if tr.get("depth") != self.trace_depth:
                raise ValueError(f"this checkpoint's trace depth {tr.get('depth')!r} differs from the agent's "
                                 f"{self.trace_depth}")
            if self.trace is not None and keys.shape[0] not in (0, self.trace.shape[0]):
                raise ValueError(f"this checkpoint holds the traces of {keys.shape[0]} lanes, the agent those of "
                                 f"{self.trace.shape[0]}")
            on_host = keys.cpu()
            n = on_host[:, 0]
            beyond = torch.arange(1, 4)[None, :] > n[:, None]
            if bool(((n < 0) | (n > self.trace_depth)).any()) or bool((on_host[:, 1:][beyond] != 0).any()):
                raise ValueError("trace keys hold a count outside 0..depth or a key beyond the count")
        car = sd.get("carousel") if self.carousel else None      # a plain staged agent ignores a file's pool
        if car is not None:
            want = tuple(self.carousel_pool.shape)
            pool, counts = (car.get("pool"), car.get("counts")) if isinstance(car, dict) else (None, None)
            if not isinstance(pool, torch.Tensor) or pool.dtype != torch.uint8 or tuple(pool.shape) != want:
                raise ValueError(f"carousel pool must be a uint8 tensor of shape {want} (stages, records per stage, 32), "
                                 f"got {getattr(pool, 'dtype', type(pool).__name__)} {tuple(getattr(pool, 'shape', ()))}")
            if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or tuple(counts.shape) != want[:1] \
                    or bool((counts < 0).any()):
                raise ValueError(f"carousel counts must be a non-negative int64 tensor of shape {want[:1]}")
        self._load_weights_and_pairs(sd, file_tiles)             # validates the rest, then writes
        if self.trace_lambda is not None:
            self._cut = None
            if tr is not None and tr["keys"].shape[0]:
                self.trace = tr["keys"].to(self.device, copy=True)
            elif self.trace is not None:
                self.trace.zero_()
        if self.carousel:
            if car is None:
                self.carousel_pool.zero_()
                self.carousel_counts.zero_()
            else:
                self.carousel_pool.copy_(car["pool"])
                self.carousel_counts.copy_(car["counts"])
            if self.carousel_fresh is not None:
                self.carousel_fresh.zero_()

    def _load_weights_and_pairs(self, sd: dict, file_tiles: tuple) -> None:
        if sd.get("kind") == self._KIND and file_tiles != self.stage_tiles:
            if not self.stage_tiles:
                raise ValueError(f"this checkpoint holds a staged network (stage_tiles {list(file_tiles)}): a plain "
                                 "BatchedNTupleAgent does not load it")
            if file_tiles:
                raise ValueError(f"this checkpoint's stage_tiles {list(file_tiles)} differ from the agent's "
                                 f"{list(self.stage_tiles)}")
            # a plain file into a staged agent: the file becomes stage 0, the later stages start at zero and take
            # its values by promotion, so every stage equals the file
            full, shape = self.weights, self._SHAPE
            try:
                self.weights, self._SHAPE = full[0], type(self)._SHAPE
                super().load_state_dict(sd)           # validates everything, then writes stage 0
            finally:
                self.weights, self._SHAPE = full, shape
            self.weights[1:].zero_()
            self.promote()
            return None
        acc = sd.get("coherence") if self.coherence is not None else None
        if acc is not None:
            if not isinstance(acc, torch.Tensor) or acc.dtype != torch.float32 or tuple(acc.shape) != self._ACC_SHAPE:
                raise ValueError(f"coherence must be a float32 tensor of shape {self._ACC_SHAPE}, got "
                                 f"{getattr(acc, 'dtype', type(acc).__name__)} {tuple(getattr(acc, 'shape', ()))}")
            E, A = acc[..., 0], acc[..., 1]
            if not bool(torch.isfinite(acc).all()):
                raise ValueError("coherence holds a value that is not finite")
            if not bool((A >= 0).all()) or not bool((E.abs() <= A).all()):
                raise ValueError("coherence holds a pair with A < 0 or |E| > A: these are not accumulators of "
                                 "q2048_nt_tc_*")
        super().load_state_dict(sd)               # validates the rest, then writes
        if self.coherence is not None:
            if acc is None:
                self.coherence.zero_()
            else:
                self.coherence.copy_(acc)


def new_stats_vectors(device):
    """The two statistics vectors as views of ONE device buffer (int64 part, then float64 part), so
    that a reader (`StatsAllReduce`) can take them with one copy."""
    raw = torch.zeros((N.NSTAT_I + N.NSTAT_F) * 8, dtype=torch.uint8, device=device)
    return raw[:N.NSTAT_I * 8].view(torch.int64), raw[N.NSTAT_I * 8:].view(torch.float64)


def stats_dict(si, sf) -> dict:
    si = np.asarray(si, dtype=np.int64)
    sf = np.asarray(sf, dtype=np.float64)
    ep = int(si[N.ST_EPISODES])
    return {
        "steps": int(si[N.ST_STEPS]), "episodes": ep, "valid_moves": int(si[N.ST_VALID]),
        "score_sum": int(si[N.ST_SCORE]), "inserts": int(si[N.ST_INSERTS]),
        "drops": int(si[N.ST_DROPS]), "explored": int(si[N.ST_EXPLORE]),
        "cas_retries": int(si[N.ST_CAS_RETRY]), "cas_fallbacks": int(si[N.ST_CAS_FALLBACK]),
        "max_tile_hist": {1 << k: int(v) for k, v in enumerate(si[N.ST_HIST0:N.ST_HIST0 + N.ST_HIST_BINS]) if v},
        "return_sum": float(sf[N.SF_RETURN]), "return_sq_sum": float(sf[N.SF_RETURN_SQ]),
        "reward_sum": float(sf[N.SF_REWARD]),
        "mean_return": float(sf[N.SF_RETURN]) / ep if ep else float("nan"),
        "mean_score": float(si[N.ST_SCORE]) / ep if ep else float("nan"),
    }


class _LazyRow:
    """The 4 Q-values of `agent.q_table[state]` (Agent/main.py:96), read back when first used: the
    lookup kernel is queued behind the update it follows and its result is fetched at the next
    synchronisation the loop makes anyway, or on first access.  Behaves like the float64 array the
    reference's dict returns (indexing, len, iteration, numpy conversion, printing)."""

    __slots__ = ("_io", "_off", "_val", "__weakref__")

    def __init__(self, io: _Staging, off: int):
        self._io, self._off, self._val = io, off, None

    def _read(self) -> None:
        if self._val is None:
            self._val = self._io.np[self._off:self._off + 16].view(np.float32).astype(np.float64)

    def _get(self) -> np.ndarray:
        if self._val is None:
            self._io.sync()                      # reads every pending row, this one included
            self._read()
        return self._val

    def __array__(self, dtype=None, copy=None):
        v = self._get()
        return v if dtype is None else v.astype(dtype)

    shape = property(lambda self: (4,))
    dtype = property(lambda self: np.dtype(np.float64))

    def __len__(self):
        return 4

    def __getitem__(self, k):
        return self._get()[k]

    def __iter__(self):
        return iter(self._get())

    def __repr__(self):
        return repr(self._get())

    def __str__(self):
        return str(self._get())

    def __getattr__(self, name):                 # tolist, max, argmax, ... : the array's own
        return getattr(self._get(), name)


class _OneStateTable:
    """`agent.q_table[state]` / `len(agent.q_table)` of the one-state adapter."""

    def __init__(self, owner: "QLearningAgent"):
        self._o = weakref.proxy(owner)

    def __getitem__(self, state) -> _LazyRow:
        o = self._o
        io, b = o._io, o._b
        off = io.take(32)                                        # [0:16] state in, [16:32] row out
        state_to_log2(state, io.np[off:off + 16])
        N.check(b._L.q2048_q_lookup(
            _ptr(b.table), b.capacity_log2, io.ptr + off, 1, 4, b.env_id0, b.flags | N.FLAG_SINGLE_ENV,
            io.ptr + off + 16, None, _ptr(b.status), _stream(b.device)), "q_lookup")
        row = _LazyRow(io, off + 16)
        io.pending.append(weakref.ref(row))
        return row

    def __len__(self) -> int:
        return self._o._b.table_size()


class QLearningAgent:
    """One-state adapter with the reference's exact surface (Agent/main.py:14-57): states are
    tuples of tuples of raw tile values, actions Python ints.  Inputs and outputs travel through a
    ring of pinned host memory that the kernels address directly (`_Staging`): choose_action is
    one launch and one synchronisation, update_q_value and q_table[state] are one launch each."""

    def __init__(self, total_epochs, action_space, learning_rate=0.1, discount_factor=0.9,
                 exploration_rate=1.0, exploration_min=0.01, capacity_log2: int = 22,
                 device="cuda", seed: int = 0, env_id: int = 0):
        self._b = BatchedQLearningAgent(total_epochs, action_space, learning_rate, discount_factor,
                                        exploration_rate, exploration_min, capacity_log2, device,
                                        seed, env_id)
        self._io = _Staging(self._b.device)
        self.q_table = _OneStateTable(self)
        self.action_space = action_space
        self.total_epochs = total_epochs

    lr = property(lambda self: self._b.lr)
    gamma = property(lambda self: self._b.gamma)
    epsilon_min = property(lambda self: self._b.epsilon_min)

    @property
    def epsilon(self) -> float:
        return self._b.epsilon

    @epsilon.setter
    def epsilon(self, v):
        self._b.epsilon = v

    def choose_action(self, state) -> int:
        io, b = self._io, self._b
        off = io.take(32)                                        # [0:16] state in, [16] action out
        state_to_log2(state, io.np[off:off + 16])
        # (the row cache only once the key set is closed: it is what carries the env's visit row from update to choose;
        # before that the plain entry points are one dependent request shorter for a single env)
        N.check(b._L.q2048_q_choose_cached(
            _ptr(b.table), b.capacity_log2, io.ptr + off, 1, 4, float(b.epsilon), b.seed, b.env_id0,
            b.ctr & 0xFFFFFFFF, b._learn_flags(), _ptr(b._cache(1)) if b.frozen else None, io.ptr + off + 16,
            _ptr(b.status), _stream(b.device)), "q_choose")
        b.ctr += 1
        io.sync()
        return int(io.np[off + 16])

    def update_q_value(self, state, action, reward, next_state, done) -> None:
        if not 0 <= int(action) <= 3:
            raise ValueError(f"action {action} outside 0..3")
        io, b = self._io, self._b
        off = io.take(48)             # [0:16] state, [16:32] next state, [32] action, [33] done, [36:40] reward
        buf = io.np
        state_to_log2(state, buf[off:off + 16])
        state_to_log2(next_state, buf[off + 16:off + 32])
        buf[off + 32], buf[off + 33] = int(action), 1 if done else 0
        buf[off + 36:off + 40].view(np.float32)[0] = reward
        b._room_for(1)                # (the table's policy -- growth, or the closed key set of one that cannot grow)
        N.check(b._L.q2048_q_update_cached(
            _ptr(b.table), b.capacity_log2, io.ptr + off, io.ptr + off + 32, io.ptr + off + 36,
            io.ptr + off + 16, io.ptr + off + 33, 1, 4, float(b.lr), float(b.gamma), b.env_id0, b._learn_flags(),
            _ptr(b._cache(1)) if b.frozen else None, _ptr(b.stats_i), _ptr(b.status), _stream(b.device)), "q_update")

    def decay_exploration(self, current_epoch) -> None:
        self._b.decay_exploration(current_epoch)
