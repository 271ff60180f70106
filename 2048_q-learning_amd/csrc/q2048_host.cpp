// q2048_host.cpp -- libq2048_host.so: the CPU twin of libq2048_hip.so.
//
// The SAME C ABI (include/q2048.h: same names, argument meaning, error codes) on HOST memory, built from
// the same per-lane arithmetic the HIP kernels inline (q2048_core.hpp / q2048_core5.hpp: SWAR slide, spawn,
// closed-form game-over, reward, Philox draws, epsilon-greedy, TD fold) and the same table: its format (keys,
// hash, bucketised probe sequence, probe limits, rows, row-cache records) is defined once, in those two headers,
// and the argument checks once, in q2048_abi.hpp -- a table trained here IS a device table, byte for byte, and
// the other way round.  Envs are split into contiguous ranges over std::threads (one thread for
// small batches); rows are claimed with a compare-and-swap on the key word and Q values written with
// 4-byte stores, as on the device -- so B = 1 (and private rows, and the deterministic step at any B) is
// the reference's sequential loop (Agent/main.py:80-109), and a shared table with several threads is the
// same Hogwild learner the fused kernel is.
//
// It is an explicit DEVICE ("cpu": `train.py --device cpu`, `BatchedGame2048Env(device="cpu")`), never a
// fallback: the package loads it only when asked for by name, and nothing of oracle/ is linked or called.
// `stream` arguments are ignored (every call is complete when it returns).  Not here: the chunked device
// allocator (q2048_table_alloc / _reserve / _grow*: Q2048_ERR_UNSUPPORTED -- host tables are the caller's
// plain memory) and, in the ROLLOUTS, the row cache as an optimisation (rows that exist are read from the table
// every time; the records a device rollout would leave are written as EMPTY ones -- what the cache carries that is
// not an optimisation IS there: the visit row of a state without a row under Q2048_FLAG_NO_NEW_ROWS, a ROWLESS
// record).  q2048_q_choose_cached / q2048_q_update_cached keep the whole cache as include/q2048.h defines it: a
// record that matches is USED instead of the table's row, and the update leaves the device's record byte for byte.
// Threads: Q2048_HOST_THREADS (default: the hardware's, at most one per 2048 envs), read at every call.
//
//   g++ -O3 -std=c++17 -fPIC -shared -pthread -I include -I 2048_q-learning_amd/csrc \
//       -o 2048_q-learning_amd/csrc/libq2048_host.so 2048_q-learning_amd/csrc/q2048_host.cpp
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <unordered_map>
#include <vector>

#include "q2048_abi.hpp"
#include "q2048_core5.hpp"

namespace {
using namespace q2048;
using u64 = unsigned long long;

constexpr int kMaxAwait = 1 << 20;

static_assert(sizeof(q2048_aux) == 16 && sizeof(q2048_slot) == 32 && sizeof(q2048_episode) == 48, "ABI layout");
static_assert(sizeof(Aux) == sizeof(q2048_aux), "core/ABI aux mismatch");

// ---- memory images of a board and its aux (the geometry Geo<N> and the table key: q2048_core5.hpp) --------------------
inline void load_board(const uint8_t* boards, int64_t i, Board& b) { std::memcpy(&b, boards + 16 * i, 16); }
inline void load_board(const uint8_t* boards, int64_t i, Board5& b) { b = board5_from_bytes(boards + 25 * i); }
inline void store_board(uint8_t* boards, int64_t i, const Board& b) { std::memcpy(boards + 16 * i, &b, 16); }
inline void store_board(uint8_t* boards, int64_t i, const Board5& b) { board5_to_bytes(b, boards + 25 * i); }
inline Aux ld_aux(const q2048_aux* aux, int64_t i) {
  Words4 w;
  std::memcpy(&w, aux + i, 16);
  return words_to_aux(w);
}
inline void st_aux(q2048_aux* aux, int64_t i, const Aux& a) {
  const Words4 w = aux_to_words(a);
  std::memcpy(aux + i, &w, 16);
}
inline void status_or(uint32_t* status, uint32_t bits) { __atomic_fetch_or(status, bits, __ATOMIC_RELAXED); }

// state keys: the shared construction (q2048_core5.hpp), with this library's way to raise TILE_OVERFLOW
template <bool SYM, class BoardT>
inline auto state_key_as(const BoardT& b, u64 salt, uint32_t* status, uint32_t& g) {
  return q2048::state_key_as<SYM>(b, salt, g, [status] { status_or(status, Q2048_STATUS_TILE_OVERFLOW); });
}
template <class BoardT>
inline auto state_key(const BoardT& b, u64 salt, uint32_t* status) {
  uint32_t g;
  return state_key_as<false>(b, salt, status, g);
}
template <int N>
inline typename Geo<N>::Key state_key_sym(bool sym, const typename Geo<N>::BoardT& b, u64 salt, uint32_t* status, uint32_t& g) {
  if constexpr (N == 4) { if (sym) return state_key_as<true>(b, salt, status, g); }
  return state_key_as<false>(b, salt, status, g);
}

// ---- the table: how this library touches it (its layout, hash and probe sequence: q2048_core.hpp) ----------------
inline u64 ld_u64(const uint64_t* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
inline float ld_f32(const float* p) {
  const uint32_t u = __atomic_load_n(reinterpret_cast<const uint32_t*>(p), __ATOMIC_RELAXED);
  return bits_f32(u);
}
inline void st_f32(float* p, float v) { __atomic_store_n(reinterpret_cast<uint32_t*>(p), f32_bits(v), __ATOMIC_RELAXED); }
inline Row ld_row(const q2048_slot* s) { return Row{ld_f32(&s->q[0]), ld_f32(&s->q[1]), ld_f32(&s->q[2]), ld_f32(&s->q[3])}; }

unsigned long long g_claim_timeouts = 0;
inline u64 await_second(const q2048_slot* s) {   // the owner of the first key word publishes the second at once
  for (int spin = 0; spin < kMaxAwait; ++spin) {
    const u64 hi = ld_u64(&s->reserved);
    if (hi != 0ull) return hi;
    if ((spin & 1023) == 1023) std::this_thread::yield();
  }
  // the owner is a host thread: on a machine with more runnable threads than CPUs it can lose its time slice between
  // its compare-and-swap and its store, for milliseconds.  A count of spins says nothing about that; wait on the clock
  // (still bounded: a protocol error ends here after two seconds, counted)
  for (const auto give_up = std::chrono::steady_clock::now() + std::chrono::seconds(2); std::chrono::steady_clock::now() < give_up;) {
    std::this_thread::sleep_for(std::chrono::microseconds(50));
    const u64 hi = ld_u64(&s->reserved);
    if (hi != 0ull) return hi;
  }
  __atomic_fetch_add(&g_claim_timeouts, 1ull, __ATOMIC_RELAXED);
  return 0ull;
}
inline bool slot_is(const q2048_slot*, const Geo<4>::Key&) { return true; }
inline bool slot_is(const q2048_slot* s, const Geo<5>::Key& key) {
  u64 hi = ld_u64(&s->reserved);
  if (hi == 0ull) hi = await_second(s);
  return hi == key.k1;
}
inline void publish(q2048_slot*, const Geo<4>::Key&) {}
inline void publish(q2048_slot* s, const Geo<5>::Key& key) { __atomic_store_n(&s->reserved, key.k1, __ATOMIC_RELEASE); }

// slot index (>= 0) when present, else ~h (h = the empty slot that ended the probe) or kNoSlot (probe limit)
template <class Key>
inline int64_t probe_find(const q2048_slot* table, u64 mask, const Key& key, Row& row, uint32_t maxp = kRolloutProbe) {
  const Seq sq = seq_of(key_hash(key), mask);
  row = Row{0.f, 0.f, 0.f, 0.f};
  for (uint32_t p = 0, lim = probe_limit(mask, maxp); p < lim; ++p) {
    const u64 i = seq_slot(sq, p);
    const u64 k = ld_u64(&table[i].key);
    if (k == 0ull) return ~(int64_t)i;
    if (k == key.k0 && slot_is(&table[i], key)) { row = ld_row(&table[i]); return (int64_t)i; }
  }
  return kNoSlot;
}
// The lookup of a 5x5 table with a closed key set from its side array of LINE SUMMARIES (q2048_table_summarise_side):
// the kernel's probe_find_summary, through the very decode it uses (q2048_core.hpp: summary_decode / summary_pop) --
// one word per line of the sequence says where the sequence ends (absent) or which slots can hold the key.  Visits the
// slots probe_find visits, in its order, under the same limit; no wait for a second key word (the key set is closed).
inline int64_t probe_find_summary(const q2048_slot* table, const uint64_t* side, u64 mask, const Geo<5>::Key& key, Row& row,
                                  uint32_t maxp = kRolloutProbe) {
  const u64 hash = key_hash(key);
  const Seq sq = seq_of(hash, mask);
  const u64 fp = summary_fp(hash);
  row = Row{0.f, 0.f, 0.f, 0.f};
  for (uint32_t p = 0, lim = probe_limit(mask, maxp); p < lim; p += 4u) {
    const u64 line = (sq.line0 + (u64)(p >> 2)) & sq.lmask;
    SummaryHits hits = summary_decode(ld_u64(&side[line]), fp, sq.off);
    uint32_t r;
    bool absent;
    while (summary_pop(hits, sq.off, r, absent)) {
      const u64 i = (line << 2) | (u64)r;
      if (absent) return ~(int64_t)i;
      if (ld_u64(&table[i].key) == key.k0 && ld_u64(&table[i].reserved) == key.k1) { row = ld_row(&table[i]); return (int64_t)i; }
    }
  }
  return kNoSlot;
}
inline int64_t probe_find_summary(const q2048_slot* table, const uint64_t*, u64 mask, const Geo<4>::Key& key, Row& row) {
  return probe_find(table, mask, key, row);   // (4x4: the in-slot summaries are written, not read, by this library)
}
// find-or-create from slot `start` of the key's sequence on
template <class Key>
inline int64_t probe_insert(q2048_slot* table, u64 mask, const Key& key, u64 start, bool& inserted,
                            uint32_t maxp = kRolloutProbe) {
  const Seq sq = seq_of(key_hash(key), mask);
  inserted = false;
  u64 i = start & mask;
  for (uint32_t p = seq_pos(sq, i), lim = probe_limit(mask, maxp); p < lim; i = seq_slot(sq, ++p)) {
    uint64_t k = ld_u64(&table[i].key);
    if (k == 0ull) {
      uint64_t expect = 0ull;
      if (__atomic_compare_exchange_n(&table[i].key, &expect, (uint64_t)key.k0, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) {
        publish(&table[i], key);
        inserted = true;
        return (int64_t)i;
      }
      k = expect;
    }
    if (k == key.k0 && slot_is(&table[i], key)) return (int64_t)i;
  }
  return kNoSlot;
}
// find, then create where the probe ended: the defaultdict's q_table[state] (Agent/main.py:16,41-43)
// (`create` = false: Q2048_FLAG_NO_NEW_ROWS -- the key set is closed, an absent state stays absent and reads as zeros)
template <class Key>
inline int64_t find_or_create(q2048_slot* table, u64 mask, const Key& key, Row& row, bool& inserted, bool create = true) {
  inserted = false;
  int64_t slot = probe_find(table, mask, key, row);
  if (slot < 0 && slot != kNoSlot && create) {
    slot = probe_insert(table, mask, key, (u64)~slot, inserted);
    if (slot >= 0 && !inserted) row = ld_row(&table[slot]);   // another thread created it meanwhile
  }
  return slot;
}

struct TdCounters { uint64_t retries = 0, fallbacks = 0; };
// update_q_value on one entry (Agent/main.py:43): one store, or (Q2048_FLAG_TD_CAS) a bounded compare-and-swap loop
inline float td_update(q2048_slot* slot, int a, float guess, float reward, float max_next, bool done, double lr,
                       double gamma, bool cas, TdCounters& c) {
  float nq = td_value(guess, reward, max_next, done, lr, gamma);
  if (!cas) { st_f32(&slot->q[a], nq); return nq; }
  uint32_t* addr = reinterpret_cast<uint32_t*>(&slot->q[a]);
  uint32_t expect = f32_bits(guess);
  for (int it = 0; it < kMaxCas; ++it) {
    if (__atomic_compare_exchange_n(addr, &expect, f32_bits(nq), false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) return nq;
    ++c.retries;
    nq = td_value(bits_f32(expect), reward, max_next, done, lr, gamma);
  }
  ++c.fallbacks;
  st_f32(&slot->q[a], nq);
  return nq;
}

// ---- visit rows (Q2048_FLAG_NO_NEW_ROWS): the device's rowless row-cache records, byte for byte ---------------------
// With the key set closed a state without a row reads as the zero row the defaultdict would have created, and while the
// env STAYS in it (invalid moves) that fresh row learns as the defaultdict's would (Agent/main.py:43); it is never part
// of the table.  Inside a call it is the lane's carried row; between calls it travels through the caller's row cache
// as a record whose slot field is all ones.  Every other record the device would write is written empty here.
inline bool rec_key_is(const RowCache<4>& r, const Geo<4>::Key& k) { return r.key == k.k0; }
inline bool rec_key_is(const RowCache<5>& r, const Geo<5>::Key& k) { return r.key == k.k0 && r.key_hi == k.k1; }
inline void rec_set_key(RowCache<4>& r, const Geo<4>::Key& k) { r.key = k.k0; }
inline void rec_set_key(RowCache<5>& r, const Geo<5>::Key& k) { r.key = k.k0; r.key_hi = k.k1; r.pad = 0; }
template <int N>
inline bool visit_get(const void* cache, int64_t i, const q2048_slot* table, u64 mask, const typename Geo<N>::Key& key, Row& row) {
  if (cache == nullptr) return false;
  const RowCache<N>& r = static_cast<const RowCache<N>*>(cache)[i];
  if (!rec_key_is(r, key) || r.slot != (kCacheRowless | cache_tag(table, mask))) return false;
  row = Row{r.q[0], r.q[1], r.q[2], r.q[3]};
  return true;
}
template <int N>
inline void visit_put(void* cache, int64_t i, const q2048_slot* table, u64 mask, const typename Geo<N>::Key& key, const Row& row,
                      bool rowless) {
  if (cache == nullptr) return;
  RowCache<N>& r = static_cast<RowCache<N>*>(cache)[i];
  std::memset(&r, 0, sizeof r);                    // an empty record (this library never reads a row through the cache)
  if (!rowless) return;
  rec_set_key(r, key);
  r.q[0] = row.q0; r.q[1] = row.q1; r.q[2] = row.q2; r.q[3] = row.q3;
  r.slot = kCacheRowless | cache_tag(table, mask);
}

// ---- the row cache of q2048_q_choose_cached / q2048_q_update_cached (include/q2048.h), as the kernels keep it ------
// A record is used when its key is the key of the board passed in AND it carries this table's tag: the row is then
// the record's (it does not see what was written to the table since) and `slot` its slot -- kNoSlot for a rowless
// record, which only a call with Q2048_FLAG_NO_NEW_ROWS accepts.
template <int N>
inline bool cache_get(const void* cache, int64_t i, const q2048_slot* table, u64 mask, const typename Geo<N>::Key& key, Row& row,
                      int64_t& slot, bool rowless_ok) {
  if (cache == nullptr) return false;
  const RowCache<N>& r = static_cast<const RowCache<N>*>(cache)[i];
  if (!rec_key_is(r, key) || (r.slot & ~kCacheSlotMask) != cache_tag(table, mask)) return false;
  const u64 v = r.slot & kCacheSlotMask;
  if (v == kCacheRowless && !rowless_ok) return false;
  slot = v == kCacheRowless ? kNoSlot : (int64_t)v;
  row = Row{r.q[0], r.q[1], r.q[2], r.q[3]};
  return true;
}
// the record an update leaves: the row read as next_state with its slot; without a row, the visit row (`rowless`)
// or nothing to remember (key 0)
inline void rec_set_hi(RowCache<4>&, const Geo<4>::Key&) {}
inline void rec_set_hi(RowCache<5>& r, const Geo<5>::Key& k) { r.key_hi = k.k1; }
template <int N>
inline void cache_put(void* cache, int64_t i, const q2048_slot* table, u64 mask, const typename Geo<N>::Key& key, const Row& row,
                      int64_t slot, bool rowless) {
  if (cache == nullptr) return;
  RowCache<N>& r = static_cast<RowCache<N>*>(cache)[i];
  std::memset(&r, 0, sizeof r);
  r.key = (slot >= 0 || rowless) ? key.k0 : 0ull;
  rec_set_hi(r, key);
  r.q[0] = row.q0; r.q[1] = row.q1; r.q[2] = row.q2; r.q[3] = row.q3;
  r.slot = (slot >= 0 ? ((u64)slot & kCacheSlotMask) : kCacheRowless) | cache_tag(table, mask);
}

// q2048_rowcache_rebind: visit rows follow their table's rows into another allocation; every other record is emptied
template <int N>
void rowcache_rebind_n(void* row_cache, int64_t B, u64 tag_from, u64 tag_to) {
  RowCache<N>* c = static_cast<RowCache<N>*>(row_cache);
  for (int64_t i = 0; i < B; ++i) {
    if (c[i].key != 0ull && c[i].slot == (kCacheRowless | tag_from)) c[i].slot = kCacheRowless | tag_to;
    else std::memset(&c[i], 0, sizeof c[i]);
  }
}

// ---- threads ---------------------------------------------------------------------------------------------------
int threads_for(int64_t B) {
  int T = 0;
  if (const char* e = std::getenv("Q2048_HOST_THREADS")) T = std::atoi(e);
  if (T <= 0) T = (int)std::thread::hardware_concurrency();
  if (T <= 0) T = 1;
  const int64_t by_work = (B + 2047) / 2048;
  if ((int64_t)T > by_work) T = (int)by_work;
  return T < 1 ? 1 : T;
}
// f(lo, hi, t) over contiguous ranges of [0, B); returns the number of ranges
template <class F>
int parallel_ranges(int64_t B, F f) {
  const int T = threads_for(B);
  if (T == 1) { f((int64_t)0, B, 0); return 1; }
  std::vector<std::thread> th;
  th.reserve((size_t)T);
  for (int t = 0; t < T; ++t) {
    const int64_t lo = B * t / T, hi = B * (t + 1) / T;
    th.emplace_back([=] { f(lo, hi, t); });
  }
  for (auto& x : th) x.join();
  return T;
}

struct Stats {
  uint64_t i[Q2048_NSTAT_I] = {};
  double f[Q2048_NSTAT_F] = {};
  void episode(const Aux& a, uint32_t max_l2) {
    i[Q2048_ST_SCORE] += (uint64_t)(int64_t)a.score;
    i[Q2048_ST_HIST0 + (max_l2 > 22u ? 22u : max_l2)] += 1;
    const double ret = (double)a.ep_return;
    f[Q2048_SF_RETURN] += ret;
    f[Q2048_SF_RETURN_SQ] += ret * ret;
  }
};
void stats_merge(const std::vector<Stats>& parts, int used, int64_t* gi, double* gf) {   // in range order: a fixed sum
  for (int t = 0; t < used; ++t) {
    if (gi != nullptr) for (int k = 0; k < Q2048_NSTAT_I; ++k) gi[k] += (int64_t)parts[(size_t)t].i[k];
    if (gf != nullptr) for (int k = 0; k < Q2048_NSTAT_F; ++k) gf[k] += parts[(size_t)t].f[k];
  }
}

inline int env_bits(uint32_t flags) {
  return ((flags & Q2048_FLAG_ENV_DQN) ? kEnvDqn : 0) | ((flags & Q2048_FLAG_RESET_SHAPING) ? kEnvResetShaping : 0);
}
template <class BoardT>
inline StepOut env_step_any(int env, BoardT& b, Aux& a, int act, uint32_t x_pos, uint32_t x_val, uint32_t y_pos, uint32_t y_val) {
  return (env & kEnvDqn) ? env_step_profile<kEnvDqn>(b, a, act, x_pos, x_val, y_pos, y_val)
                         : env_step_profile<0>(b, a, act, x_pos, x_val, y_pos, y_val);
}
// the fused rollout's step: the reward tables read from one image (as the device's workgroups read theirs from LDS)
const LutImage g_lut_image = Q2048_LUT_IMAGE;
template <class BoardT>
inline StepOut env_step_any(int env, BoardT& b, Aux& a, int act, uint32_t x_pos, uint32_t x_val, uint32_t y_pos, uint32_t y_val,
                            const ImageLuts& lut) {
  return (env & kEnvDqn) ? env_step_profile<kEnvDqn>(b, a, act, x_pos, x_val, y_pos, y_val, lut)
                         : env_step_profile<0>(b, a, act, x_pos, x_val, y_pos, y_val, lut);
}

// ---- env ---------------------------------------------------------------------------------------------------------
template <int N>
void env_init_impl(uint8_t* boards, q2048_aux* aux, int64_t B, uint64_t seed, uint64_t env_id0) {
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      typename Geo<N>::BoardT b;
      Aux a;
      init_env(b, a, seed, env_id0 + (uint64_t)i);
      store_board(boards, i, b);
      st_aux(aux, i, a);
    }
  });
}
template <int N>
void env_reset_impl(uint8_t* boards, q2048_aux* aux, const uint8_t* mask, int64_t B, uint64_t seed, uint64_t env_id0,
                    uint32_t flags) {
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      if (mask != nullptr && mask[i] == 0) continue;
      typename Geo<N>::BoardT b;
      load_board(boards, i, b);
      Aux a = ld_aux(aux, i);
      begin_episode(b, a, seed, env_id0 + (uint64_t)i, (flags & Q2048_FLAG_RESET_SHAPING) != 0);
      store_board(boards, i, b);
      st_aux(aux, i, a);
    }
  });
}
template <int N>
void env_step_impl_n(const uint8_t* boards_in, uint8_t* boards, q2048_aux* aux, const uint8_t* actions, int64_t B,
                     uint64_t seed, uint64_t env_id0, uint32_t ctr, uint32_t flags, float* reward, uint8_t* done,
                     uint8_t* max_l2, int32_t* max_tile, uint32_t* status, const uint32_t* draw_pos,
                     const uint32_t* draw_val, const uint32_t* draw_opos, const uint32_t* draw_oval, int stride) {
  const int env = env_bits(flags);
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      typename Geo<N>::BoardT b;
      load_board(boards_in, i, b);
      const int act = actions[i];
      if (act > 3) {   // rejected, never masked (Game2048_env.py:56-60 would mis-rotate)
        status_or(status, Q2048_STATUS_BAD_ACTION);
        reward[i] = 0.f; done[i] = 0; max_l2[i] = 0;
        if (max_tile != nullptr) max_tile[i] = 0;
        if (boards != boards_in) store_board(boards, i, b);
        continue;
      }
      Aux a = ld_aux(aux, i);
      Draws x{0u, 0u, 0u, 0u}, y{0u, 0u, 0u, 0u};
      if (draw_pos != nullptr) {
        x.x2 = draw_pos[i * stride]; x.x3 = draw_val[i * stride];
        if (env & kEnvDqn) { y.x0 = draw_opos[i * stride]; y.x1 = draw_oval[i * stride]; }
      } else {
        x = draws(seed, env_id0 + (uint64_t)i, ctr, kStreamStep);
        if (env & kEnvDqn) y = draws(seed, env_id0 + (uint64_t)i, ctr, kStreamOver);
      }
      const StepOut o = env_step_any(env, b, a, act, x.x2, x.x3, y.x0, y.x1);
      store_board(boards, i, b);
      st_aux(aux, i, a);
      reward[i] = o.reward; done[i] = o.done; max_l2[i] = o.max_log2;
      if (max_tile != nullptr) max_tile[i] = o.max_log2 ? (int32_t)(1u << o.max_log2) : 0;
    }
  });
}
int env_step_impl(const uint8_t* boards_in, uint8_t* boards, q2048_aux* aux, const uint8_t* actions, int64_t B, int n,
                  uint64_t seed, uint64_t env_id0, uint32_t ctr, uint32_t flags, float* reward, uint8_t* done,
                  uint8_t* max_l2, int32_t* max_tile, uint32_t* status, const uint32_t* draw_pos,
                  const uint32_t* draw_val, const uint32_t* draw_opos, const uint32_t* draw_oval, int stride) {
  if (int e = check_batch(B, n)) return e;
  if (int e = check_flags(flags)) return e;
  if (!boards_in || !boards || !aux || !actions || !reward || !done || !max_l2 || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards_in) || !aligned16(boards) || !aligned16(aux)) return Q2048_ERR_ALIGN;
  if (boards_in != boards) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(boards_in), a1 = reinterpret_cast<uintptr_t>(boards);
    const uintptr_t len = (uintptr_t)B * (uintptr_t)(n * n);
    if (a0 < a1 + len && a1 < a0 + len) return Q2048_ERR_ALIGN;
  }
  if (B == 0) return Q2048_OK;
  if (n == 4) env_step_impl_n<4>(boards_in, boards, aux, actions, B, seed, env_id0, ctr, flags, reward, done, max_l2,
                                 max_tile, status, draw_pos, draw_val, draw_opos, draw_oval, stride);
  else env_step_impl_n<5>(boards_in, boards, aux, actions, B, seed, env_id0, ctr, flags, reward, done, max_l2,
                          max_tile, status, draw_pos, draw_val, draw_opos, draw_oval, stride);
  return Q2048_OK;
}

// ---- agent -------------------------------------------------------------------------------------------------------
template <int N>
void q_choose_impl_n(const q2048_slot* table, u64 mask, const uint8_t* boards, int64_t B, double eps, uint64_t seed,
                     uint64_t env_id0, uint32_t ctr, uint32_t flags, uint8_t* actions, uint32_t* status,
                     const uint32_t* draw_eps, const uint32_t* draw_act, const void* cache) {
  const bool frozen = (flags & Q2048_FLAG_NO_NEW_ROWS) != 0;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      typename Geo<N>::BoardT b;
      load_board(boards, i, b);
      const uint64_t id = env_id0 + (uint64_t)i;
      const u64 salt = (flags & Q2048_FLAG_INDEPENDENT) ? lane_salt(id) : 0ull;
      Draws x;
      if (draw_eps != nullptr) { x.x0 = draw_eps[i]; x.x1 = draw_act[i]; }
      else x = draws(seed, id, ctr, kStreamStep);
      int act;
      if (draw_uniform(x.x0) < eps) act = draw_action(x.x1);      // Agent/main.py:35-36: no table access when exploring
      else {
        Row r;
        const auto key = state_key(b, salt, status);
        int64_t slot;
        // the env's record (closed key set: also its visit row), else the table
        if (!cache_get<N>(cache, i, table, mask, key, r, slot, frozen)) probe_find(table, mask, key, r);
        act = argmax4(r.q0, r.q1, r.q2, r.q3);
      }
      actions[i] = (uint8_t)act;
    }
  });
}
int q_choose_impl(const q2048_slot* table, int cap_log2, const uint8_t* boards, int64_t B, int n, double eps,
                  uint64_t seed, uint64_t env_id0, uint32_t ctr, uint32_t flags, const void* row_cache,
                  uint8_t* actions, uint32_t* status, const uint32_t* draw_eps, const uint32_t* draw_act) {
  if (int e = check_batch(B, n)) return e;
  if (int e = check_flags(flags)) return e;
  if (int e = check_table(table, cap_log2)) return e;
  if (!boards || !actions || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(row_cache)) return Q2048_ERR_ALIGN;
  if (!(eps >= 0.0 && eps <= 1.0)) return Q2048_ERR_RANGE;
  if (B == 0) return Q2048_OK;
  const u64 mask = (1ull << cap_log2) - 1ull;
  if (n == 4) q_choose_impl_n<4>(table, mask, boards, B, eps, seed, env_id0, ctr, flags, actions, status, draw_eps, draw_act, row_cache);
  else q_choose_impl_n<5>(table, mask, boards, B, eps, seed, env_id0, ctr, flags, actions, status, draw_eps, draw_act, row_cache);
  return Q2048_OK;
}

template <int N>
void q_update_impl_n(q2048_slot* table, u64 mask, const uint8_t* s, const uint8_t* actions, const float* reward,
                     const uint8_t* s2, const uint8_t* done, int64_t B, double lr, double gamma, uint64_t env_id0,
                     uint32_t flags, int64_t* stats_i, uint32_t* status, void* cache) {
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const bool cas = (flags & Q2048_FLAG_TD_CAS) != 0, create = (flags & Q2048_FLAG_NO_NEW_ROWS) == 0;
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int t) {
    Stats& st = sp[t];
    TdCounters tdc;
    for (int64_t i = lo; i < hi; ++i) {
      const int act = actions[i];
      if (act > 3) { status_or(status, Q2048_STATUS_BAD_ACTION); continue; }
      typename Geo<N>::BoardT b_s, b_n;
      load_board(s, i, b_s);
      load_board(s2, i, b_n);
      const u64 salt = (flags & Q2048_FLAG_INDEPENDENT) ? lane_salt(env_id0 + (uint64_t)i) : 0ull;
      const auto key_s = state_key(b_s, salt, status);
      const auto key_n = state_key(b_n, salt, status);
      Row rs, rn;
      bool ins_s = false, ins_n = false;
      // q_table[state] (:43): the row this env carried over from its last update (closed key set: or its visit row),
      // else the table's, created when absent
      int64_t slot = kNoSlot;
      if (!cache_get<N>(cache, i, table, mask, key_s, rs, slot, !create)) slot = find_or_create(table, mask, key_s, rs, ins_s, create);
      rn = rs;
      const bool same = key_eq(key_n, key_s);
      int64_t slot_n = slot;
      if (!same) slot_n = find_or_create(table, mask, key_n, rn, ins_n, create);     // q_table[next_state] (:41)
      st.i[Q2048_ST_INSERTS] += (uint64_t)ins_s + (uint64_t)ins_n;
      const float max_next = max4(rn.q0, rn.q1, rn.q2, rn.q3);
      if (slot >= 0) {
        const float nq = td_update(&table[slot], act, row_get(rs, act), reward[i], max_next, done[i] != 0, lr, gamma, cas, tdc);
        if (same) row_set(rn, act, nq);                           // the row it stays on just changed (:100)
      } else {
        st.i[Q2048_ST_DROPS] += 1;
        if (create) status_or(status, Q2048_STATUS_TABLE_FULL);   // (closed key set: the caller's policy)
        else if (same) row_set(rn, act, td_value(row_get(rs, act), reward[i], max_next, done[i] != 0, lr, gamma));
      }
      cache_put<N>(cache, i, table, mask, key_n, rn, slot_n, !create);
    }
    st.i[Q2048_ST_CAS_RETRY] += tdc.retries;
    st.i[Q2048_ST_CAS_FALLBACK] += tdc.fallbacks;
  });
  stats_merge(parts, used, stats_i, nullptr);
}

template <int N>
void q_lookup_impl_n(const q2048_slot* table, u64 mask, const uint8_t* boards, int64_t B, uint64_t env_id0,
                     uint32_t flags, float* q_out, uint8_t* found, uint32_t* status) {
  const bool sym = (flags & Q2048_FLAG_SYMMETRIC) != 0;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      typename Geo<N>::BoardT b;
      load_board(boards, i, b);
      const uint64_t id = (flags & Q2048_FLAG_SINGLE_ENV) ? env_id0 : env_id0 + (uint64_t)i;
      const u64 salt = (flags & Q2048_FLAG_INDEPENDENT) ? lane_salt(id) : 0ull;
      Row r;
      uint32_t g;
      const int64_t slot = probe_find(table, mask, state_key_sym<N>(sym, b, salt, status, g), r, kMaxProbe);
      if (sym) r = row_env(r, g);                      // q_out is in the env's frame
      q_out[4 * i] = r.q0; q_out[4 * i + 1] = r.q1; q_out[4 * i + 2] = r.q2; q_out[4 * i + 3] = r.q3;
      if (found != nullptr) found[i] = slot >= 0;
    }
  });
}

// ---- the fused rollout: Agent/main.py:91-101 + the reset of :81, `steps` times per env ----------------------------
// A thread walks its range in GROUPS of kGroup envs, step by step: first every env of the group chooses, steps
// and asks for the cache line its next state's row starts on (a prefetch), then every env does its table work.
// One env at a time, every probe of s' is a DRAM miss the core sits through (~100 ns against ~100 ns of
// arithmetic per step); sixteen at a time the misses overlap.  Per env nothing changes -- the same calls in the
// same order on the same draws -- so B = 1 and private rows are the reference's loop as before; on a shared table
// the interleaving of envs is a different schedule of the same Hogwild learner.
constexpr int kGroup = 16;
template <int N>
void fused_rollout_n(uint8_t* boards, q2048_aux* aux, q2048_slot* table, u64 mask, int64_t B, int steps, double eps,
                     double lr, double gamma, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                     int64_t* stats_i, double* stats_f, uint32_t* status, q2048_episode* log, int64_t log_cap,
                     uint64_t* log_count, void* cache, const uint64_t* side) {
  using BoardT = typename Geo<N>::BoardT;
  using Key = typename Geo<N>::Key;
  struct Lane {
    BoardT b; Aux a; Key key_s, key_n; Row q; int64_t slot_s; u64 salt; uint64_t id; double reward_sum;
    StepOut o; int act; bool explored, same; DrawPrep prep;
    uint32_t g_s, g_n;      // Q2048_FLAG_SYMMETRIC: which image of the board the canonical one is (else 0)
  };
  const uint64_t eps_t = eps_threshold(eps);     // the step's epsilon test and draws as the device kernel does them
  const ImageLuts lut{&g_lut_image};
  const int env = env_bits(flags);
  const bool play_only = (flags & Q2048_FLAG_PLAY_ONLY) != 0, no_learn = (flags & Q2048_FLAG_NO_LEARN) != 0;
  const bool learns = !play_only && !no_learn, frozen = (flags & Q2048_FLAG_NO_NEW_ROWS) != 0;
  const bool creates = learns && !frozen, cas = (flags & Q2048_FLAG_TD_CAS) != 0;
  // Q2048_FLAG_SYMMETRIC: keys, the carried row, the visit row and every table index are in the canonical frame;
  // only the four values handed to the epsilon-greedy choice and the action's index into the row are permuted
  const bool sym = N == 4 && !play_only && (flags & Q2048_FLAG_SYMMETRIC) != 0;
  // 5x5, key set closed, Q2048_FLAG_LINE_SUMMARY and a side array: the lookups are decided from it, as on the device
  const bool summary = N == 5 && learns && frozen && (flags & Q2048_FLAG_LINE_SUMMARY) != 0 && side != nullptr;
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
    auto find = [=](const Key& key, Row& row) {
      return summary ? probe_find_summary(table, side, mask, key, row) : probe_find(table, mask, key, row);
    };
    Stats& st = sp[tid];
    TdCounters tdc;
    bool any_drop = false;
    Lane lane[kGroup];
    for (int64_t g0 = lo; g0 < hi; g0 += kGroup) {
      const int n = (int)(hi - g0 < kGroup ? hi - g0 : kGroup);
      for (int l = 0; l < n; ++l) {
        Lane& L = lane[l];
        const int64_t i = g0 + l;
        L.id = env_id0 + (uint64_t)i;
        L.salt = (flags & Q2048_FLAG_INDEPENDENT) ? lane_salt(L.id) : 0ull;
        load_board(boards, i, L.b);
        L.a = ld_aux(aux, i);
        L.key_s = state_key_sym<N>(sym, L.b, L.salt, status, L.g_s);
        // the row of the current state: read when the state is reached and carried (as the kernel carries it in
        // registers); created at its first update (the defaultdict creates q_table[state] at :43)
        L.q = Row{0.f, 0.f, 0.f, 0.f};
        L.slot_s = play_only ? kNoSlot : find(L.key_s, L.q);
        if (frozen && learns && L.slot_s < 0) visit_get<N>(cache, i, table, mask, L.key_s, L.q);   // the visit row goes on
        L.reward_sum = 0.0;
        L.prep = draws_prepare(seed, L.id, kStreamStep);
      }
      for (int t = 0; t < steps; ++t) {
        for (int l = 0; l < n; ++l) {                    // choose, step, ask for s'
          Lane& L = lane[l];
          const Draws x = draws_at(L.prep, ctr0 + (uint32_t)t);
          Draws y{0u, 0u, 0u, 0u};
          if (env & kEnvDqn) y = draws(seed, L.id, ctr0 + (uint32_t)t, kStreamOver);
          const Row qe = sym ? row_env(L.q, L.g_s) : L.q;
          L.act = eps_greedy_at(eps_t, x.x0, x.x1, qe.q0, qe.q1, qe.q2, qe.q3, L.explored);      // :92
          L.o = env_step_any(env, L.b, L.a, L.act, x.x2, x.x3, y.x0, y.x1, lut);                 // :93
          L.key_n = state_key_sym<N>(sym, L.b, L.salt, status, L.g_n);                           // :94
          // (symmetric: still "the move was invalid" -- a valid move adds a spawned tile, so the tile sum grows and
          // s' can never lie in the orbit of s)
          L.same = key_eq(L.key_n, L.key_s);
          if (!L.same && !play_only) __builtin_prefetch(&table[key_hash(L.key_n) & mask], 1, 1);
        }
        for (int l = 0; l < n; ++l) {                    // the table: q_table[next_state], the TD write, the reset
          Lane& L = lane[l];
          const StepOut& o = L.o;
          const int act = sym ? sym_action(L.g_s, L.act) : L.act;   // the action's index into the (canonical) row
          bool ins_s = false, ins_n = false;
          if (L.slot_s < 0 && L.slot_s != kNoSlot && creates) L.slot_s = probe_insert(table, mask, L.key_s, (u64)~L.slot_s, ins_s);
          Row qn = L.q;                                                                          // q_table[next_state] (:41)
          int64_t slot_n = L.slot_s;
          if (!L.same) {
            if (play_only) { qn = Row{0.f, 0.f, 0.f, 0.f}; slot_n = kNoSlot; }
            else if (creates) slot_n = find_or_create(table, mask, L.key_n, qn, ins_n);
            else slot_n = find(L.key_n, qn);
          }
          const float max_next = max4(qn.q0, qn.q1, qn.q2, qn.q3);
          const bool updated = L.slot_s >= 0;
          float nq = 0.f;
          if (updated) {                                                                         // :43, :99
            if (no_learn) nq = td_value(row_get(L.q, act), o.reward, max_next, o.done != 0, lr, gamma);
            else nq = td_update(&table[L.slot_s], act, row_get(L.q, act), o.reward, max_next, o.done != 0, lr, gamma, cas, tdc);
          } else if (frozen && learns) {   // closed key set, no row: the update lands in the visit row (the carried L.q)
            nq = td_value(row_get(L.q, act), o.reward, max_next, o.done != 0, lr, gamma);
          }
          st.i[Q2048_ST_VALID] += o.valid != 0;
          st.i[Q2048_ST_EXPLORE] += L.explored;
          st.i[Q2048_ST_INSERTS] += (uint64_t)ins_s + (uint64_t)ins_n;
          if (!updated && learns) { st.i[Q2048_ST_DROPS] += 1; any_drop = any_drop || !frozen; }
          L.reward_sum += (double)o.reward;
          if (o.done) {                                                                          // :103
            st.i[Q2048_ST_EPISODES] += 1;
            st.episode(L.a, o.max_log2);
            if (log != nullptr) {                                                                // :59-62, :105
              const uint64_t at = __atomic_fetch_add(log_count, (uint64_t)1, __ATOMIC_RELAXED);
              if ((int64_t)at < log_cap) {
                Row ql = L.q;
                if ((updated || (frozen && learns)) && !no_learn) row_set(ql, act, nq);
                q2048_episode rec;
                if (sym) ql = row_env(ql, L.g_s);             // the log is the env's view
                rec.env_id = L.id; rec.episode = L.a.episode; rec.action = (uint8_t)L.act;
                rec.max_log2 = o.max_log2; rec.steps_lo = (uint16_t)(ctr0 + (uint32_t)t);
                rec.reward = o.reward; rec.total_return = L.a.ep_return; rec.score = L.a.score;
                rec.q[0] = ql.q0; rec.q[1] = ql.q1; rec.q[2] = ql.q2; rec.q[3] = ql.q3;
                rec.reserved = 0u;
                log[at] = rec;
              }
            }
            begin_episode(L.b, L.a, seed, L.id, (env & kEnvResetShaping) != 0);                  // :81
            L.key_s = state_key_sym<N>(sym, L.b, L.salt, status, L.g_s);
            L.q = Row{0.f, 0.f, 0.f, 0.f};
            L.slot_s = play_only ? kNoSlot : find(L.key_s, L.q);
          } else if (L.same) {           // invalid move: same state, its row just changed (:100)
            if ((updated || (frozen && learns)) && !no_learn) row_set(L.q, act, nq);
            else if (!updated) L.slot_s = kNoSlot;
          } else {
            L.key_s = L.key_n; L.slot_s = slot_n; L.q = qn; L.g_s = L.g_n;                       // :100
          }
        }
      }
      for (int l = 0; l < n; ++l) {
        st.i[Q2048_ST_STEPS] += (uint64_t)steps;
        st.f[Q2048_SF_REWARD] += lane[l].reward_sum;
        store_board(boards, g0 + l, lane[l].b);
        st_aux(aux, g0 + l, lane[l].a);
        if (!play_only) visit_put<N>(cache, g0 + l, table, mask, lane[l].key_s, lane[l].q, frozen && learns && lane[l].slot_s < 0);
      }
    }
    st.i[Q2048_ST_CAS_RETRY] += tdc.retries;
    st.i[Q2048_ST_CAS_FALLBACK] += tdc.fallbacks;
    if (any_drop) status_or(status, Q2048_STATUS_TABLE_FULL);
  });
  stats_merge(parts, used, stats_i, stats_f);
}

// ---- the greedy player (q2048_play_rollout): row, legal-move mask, play_action (q2048_core.hpp: the kernel's own
// decision), env step, statistics and reset on done -- `steps` times per env, the table only read.  Envs are split
// over the threads as the fused rollout splits them; an env's trajectory does not depend on the split.
template <int N>
void play_rollout_n(uint8_t* boards, q2048_aux* aux, const q2048_slot* table, u64 mask, int64_t B, int steps, double eps,
                    uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t* stats_i, double* stats_f,
                    uint32_t* status) {
  const uint64_t eps_t = eps_threshold(eps);
  const ImageLuts lut{&g_lut_image};
  const int env = env_bits(flags);
  const bool sym = (flags & Q2048_FLAG_SYMMETRIC) != 0;
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
    Stats& st = sp[tid];
    for (int64_t i = lo; i < hi; ++i) {
      const uint64_t id = env_id0 + (uint64_t)i;
      const u64 salt = (flags & Q2048_FLAG_INDEPENDENT) ? lane_salt(id) : 0ull;
      typename Geo<N>::BoardT b;
      load_board(boards, i, b);
      Aux a = ld_aux(aux, i);
      const DrawPrep prep = draws_prepare(seed, id, kStreamStep);
      double reward_sum = 0.0;
      for (int t = 0; t < steps; ++t) {
        const Draws x = draws_at(prep, ctr0 + (uint32_t)t);
        Draws y{0u, 0u, 0u, 0u};
        if (env & kEnvDqn) y = draws(seed, id, ctr0 + (uint32_t)t, kStreamOver);
        Row q;
        uint32_t g;
        probe_find(table, mask, state_key_sym<N>(sym, b, salt, status, g), q, kMaxProbe);
        if (sym) q = row_env(q, g);                    // the legal mask and the tie order are the env's
        bool explored;
        const int act = play_action(legal_mask(b), q.q0, q.q1, q.q2, q.q3, eps_t, x.x0, x.x1, explored);
        const StepOut o = env_step_any(env, b, a, act, x.x2, x.x3, y.x0, y.x1, lut);
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        reward_sum += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          begin_episode(b, a, seed, id, (env & kEnvResetShaping) != 0);
        }
      }
      st.i[Q2048_ST_STEPS] += (uint64_t)steps;
      st.f[Q2048_SF_REWARD] += reward_sum;
      store_board(boards, i, b);
      st_aux(aux, i, a);
    }
  });
  stats_merge(parts, used, stats_i, stats_f);
}

// ---- the deterministic step: phase 1 over every env against the step-start table, then each (row, action) group
// folds its updates in env order in double and rounds once (include/q2048.h "Deterministic mode") ----------------
template <int N>
void det_rollout_n(uint8_t* boards, q2048_aux* aux, q2048_slot* table, u64 mask, int64_t B, int64_t steps, double eps,
                   double lr, double gamma, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                   int64_t* stats_i, double* stats_f, uint32_t* status, void* row_cache) {
  const int env = env_bits(flags);
  const bool create = (flags & Q2048_FLAG_NO_NEW_ROWS) == 0;
  void* const cache = create ? nullptr : row_cache;   // visit rows: closed key set only
  std::vector<int64_t> cell((size_t)B);          // slot * 4 + action, or -1 (dropped)
  std::vector<double> target((size_t)B);
  int64_t* cp = cell.data();
  double* tp = target.data();
  const int T = threads_for(B);
  for (int64_t t = 0; t < steps; ++t) {
    std::vector<Stats> parts((size_t)T);
    Stats* sp = parts.data();
    const uint32_t ctr = ctr0 + (uint32_t)t;
    const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
      Stats& st = sp[tid];
      for (int64_t i = lo; i < hi; ++i) {
        const uint64_t id = env_id0 + (uint64_t)i;
        const u64 salt = (flags & Q2048_FLAG_INDEPENDENT) ? lane_salt(id) : 0ull;
        typename Geo<N>::BoardT b;
        load_board(boards, i, b);
        Aux a = ld_aux(aux, i);
        const auto key_s = state_key(b, salt, status);
        const Draws x = draws(seed, id, ctr, kStreamStep);
        Draws y{0u, 0u, 0u, 0u};
        if (env & kEnvDqn) y = draws(seed, id, ctr, kStreamOver);
        Row q, qn;
        bool ins_s = false, ins_n = false, explored;
        const int64_t slot_s = find_or_create(table, mask, key_s, q, ins_s, create);
        const bool dropped = slot_s < 0;
        if (dropped) { q = Row{0.f, 0.f, 0.f, 0.f}; if (create || slot_s == kNoSlot) status_or(status, Q2048_STATUS_TABLE_FULL); }
        if (dropped) visit_get<N>(cache, i, table, mask, key_s, q);                          // the env's visit row
        const int act = eps_greedy(eps, x.x0, x.x1, q.q0, q.q1, q.q2, q.q3, explored);       // :92
        const StepOut o = env_step_any(env, b, a, act, x.x2, x.x3, y.x0, y.x1);              // :93
        const auto key_n = state_key(b, salt, status);
        find_or_create(table, mask, key_n, qn, ins_n, create);                               // :41
        if (cache != nullptr) {
          // a visit row is one env's: its update needs no ordering and is applied here, not by phase 2
          const bool stays = dropped && key_eq(key_n, key_s);
          if (stays) qn = q;
          Row v = q;
          if (stays && !o.done)
            row_set(v, act, td_value(row_get(q, act), o.reward, max4(qn.q0, qn.q1, qn.q2, qn.q3), false, lr, gamma));
          visit_put<N>(cache, i, table, mask, key_s, v, stays && !o.done);
        }
        cp[i] = dropped ? -1 : slot_s * 4 + act;
        tp[i] = td_target(o.reward, max4(qn.q0, qn.q1, qn.q2, qn.q3), o.done != 0, gamma);   // :42
        st.i[Q2048_ST_STEPS] += 1;
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        st.i[Q2048_ST_INSERTS] += (uint64_t)ins_s + (uint64_t)ins_n;
        st.i[Q2048_ST_DROPS] += dropped;
        st.f[Q2048_SF_REWARD] += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          begin_episode(b, a, seed, id, (env & kEnvResetShaping) != 0);
        }
        store_board(boards, i, b);
        st_aux(aux, i, a);
      }
    });
    stats_merge(parts, used, stats_i, stats_f);
    // phase 2: env order, one running double per (row, action), one rounding per group and step (:43)
    std::unordered_map<int64_t, double> run;
    run.reserve((size_t)B);
    for (int64_t i = 0; i < B; ++i) {
      if (cp[i] < 0) continue;
      auto it = run.find(cp[i]);
      if (it == run.end()) it = run.emplace(cp[i], (double)table[cp[i] >> 2].q[cp[i] & 3]).first;
      it->second = td_fold(it->second, tp[i], lr);
    }
    for (const auto& kv : run) table[kv.first >> 2].q[kv.first & 3] = (float)kv.second;
  }
}

// ---- row-tuple linear Q (BASELINE configs[1]): W = float[4][65536][4] --------------------------------------------
struct RtRows { Row e[4]; };
inline float* rt_entry(float* w, int r, uint32_t idx) { return w + (((size_t)r * kRtIdx + idx) << 2); }
inline RtRows rt_gather(const float* w, const Board& b) {
  const uint32_t idx[4] = {pack_row(b.r0), pack_row(b.r1), pack_row(b.r2), pack_row(b.r3)};
  RtRows e;
  for (int r = 0; r < 4; ++r) {
    const float* p = rt_entry(const_cast<float*>(w), r, idx[r]);
    e.e[r] = Row{ld_f32(p), ld_f32(p + 1), ld_f32(p + 2), ld_f32(p + 3)};
  }
  return e;
}
inline Row rt_q(const RtRows& e) {
  return Row{rt_sum(e.e[0].q0, e.e[1].q0, e.e[2].q0, e.e[3].q0), rt_sum(e.e[0].q1, e.e[1].q1, e.e[2].q1, e.e[3].q1),
             rt_sum(e.e[0].q2, e.e[1].q2, e.e[2].q2, e.e[3].q2), rt_sum(e.e[0].q3, e.e[1].q3, e.e[2].q3, e.e[3].q3)};
}
inline void rt_scatter(float* w, const Board& b, const RtRows& e, int act, float d) {
  const uint32_t idx[4] = {pack_row(b.r0), pack_row(b.r1), pack_row(b.r2), pack_row(b.r3)};
  for (int r = 0; r < 4; ++r) st_f32(rt_entry(w, r, idx[r]) + act, row_get(e.e[r], act) + d);
}

// ---- line-tuple linear Q (rows and columns as features): W = float[8][65536][4] ----------------------------------
struct LtRows { Row e[kLtFeatures]; };
inline LtRows lt_gather(const float* w, const LtIdx& x) {
  LtRows e;
  for (int f = 0; f < kLtFeatures; ++f) {
    const float* p = rt_entry(const_cast<float*>(w), f, x.i[f]);
    e.e[f] = Row{ld_f32(p), ld_f32(p + 1), ld_f32(p + 2), ld_f32(p + 3)};
  }
  return e;
}
inline Row lt_q(const LtRows& e) {
  return Row{lt_sum(e.e[0].q0, e.e[1].q0, e.e[2].q0, e.e[3].q0, e.e[4].q0, e.e[5].q0, e.e[6].q0, e.e[7].q0),
             lt_sum(e.e[0].q1, e.e[1].q1, e.e[2].q1, e.e[3].q1, e.e[4].q1, e.e[5].q1, e.e[6].q1, e.e[7].q1),
             lt_sum(e.e[0].q2, e.e[1].q2, e.e[2].q2, e.e[3].q2, e.e[4].q2, e.e[5].q2, e.e[6].q2, e.e[7].q2),
             lt_sum(e.e[0].q3, e.e[1].q3, e.e[2].q3, e.e[3].q3, e.e[4].q3, e.e[5].q3, e.e[6].q3, e.e[7].q3)};
}
inline void lt_scatter(float* w, const LtIdx& x, const LtRows& e, int act, float d) {
  for (int f = 0; f < kLtFeatures; ++f) st_f32(rt_entry(w, f, x.i[f]) + act, row_get(e.e[f], act) + d);
}

// ---- afterstate value learner on the line features: V = float[8][65536] -------------------------------------------
inline float* av_entry(float* v, int f, uint32_t idx) { return v + ((size_t)f * kRtIdx + idx); }
inline AvEval av_eval(const float* v, const Board& s) {
  AvEval ev;
  ev.c = av_candidates(s);
  for (int a = 0; a < 4; ++a)
    for (int f = 0; f < kLtFeatures; ++f) ev.e[a][f] = ld_f32(av_entry(const_cast<float*>(v), f, ev.c.x[a].i[f]));
  return ev;
}
inline void av_gather8(const float* v, AvTaken& t) {
  for (int f = 0; f < kLtFeatures; ++f) t.e[f] = ld_f32(av_entry(const_cast<float*>(v), f, t.x.i[f]));
}
inline void av_scatter(float* v, const AvTaken& t, float d) {
  for (int f = 0; f < kLtFeatures; ++f) st_f32(av_entry(v, f, t.x.i[f]), t.e[f] + d);
}

// ---- 6-tuple afterstate network: V = float[4][2^24]; how nt_gather / nt_eval / nt_td reach an entry here ----------
struct NtLd {
  const float* v;
  float operator()(int p, uint32_t idx) const { return ld_f32(v + ((size_t)p * kNtIdx + idx)); }
};
struct NtSt {
  float* v;
  void operator()(int p, uint32_t idx, float x) const { st_f32(v + ((size_t)p * kNtIdx + idx), x); }
};
// the pair {S, C} of acc = uint64_t[4][2^24][2] (q2048_nt_sync_*): relaxed 64-bit atomics, as on the device
struct NtSyncAdd {
  uint64_t* acc;
  void operator()(int p, uint32_t idx, int64_t q) const {
    uint64_t* e = acc + 2 * ((size_t)p * kNtIdx + idx);
    __atomic_fetch_add(e, (uint64_t)q, __ATOMIC_RELAXED);
    __atomic_fetch_add(e + 1, (uint64_t)1, __ATOMIC_RELAXED);
  }
};
struct NtSyncClaim {
  uint64_t* acc;
  uint64_t operator()(int p, uint32_t idx) const {
    return __atomic_exchange_n(acc + 2 * ((size_t)p * kNtIdx + idx) + 1, (uint64_t)0, __ATOMIC_RELAXED);
  }
};
struct NtSyncTake {
  uint64_t* acc;
  int64_t operator()(int p, uint32_t idx) const {
    return (int64_t)__atomic_exchange_n(acc + 2 * ((size_t)p * kNtIdx + idx), (uint64_t)0, __ATOMIC_RELAXED);
  }
};
// a pair {E, A} of acc = float[4][2^24][2]: one relaxed 64-bit atomic each way, packed through memcpy (a struct of two
// floats may be split into two accesses by the compiler)
struct NtTcLd {
  const float* acc;
  NtPair operator()(int p, uint32_t idx) const {
    const uint64_t w = __atomic_load_n(reinterpret_cast<const uint64_t*>(acc) + ((size_t)p * kNtIdx + idx), __ATOMIC_RELAXED);
    float f[2];
    std::memcpy(f, &w, sizeof w);
    return NtPair{f[0], f[1]};
  }
};
struct NtTcSt {
  float* acc;
  void operator()(int p, uint32_t idx, const NtPair& h) const {
    const float f[2] = {h.E, h.A};
    uint64_t w;
    std::memcpy(&w, f, sizeof w);
    __atomic_store_n(reinterpret_cast<uint64_t*>(acc) + ((size_t)p * kNtIdx + idx), w, __ATOMIC_RELAXED);
  }
};

// ---- the row evaluators of the weight families, one per family, holding what the family needs: the row and the
// legal-move mask of a board, what a player hands to play_action.  (search_best_of of it is what search_row asks for at
// every live node.)
// the staged network: the table of a stage
struct NtsLdOf {
  const float* v;
  NtLd operator()(uint32_t stage) const { return NtLd{v + (size_t)stage * kNtsStageFloats}; }
};
struct NtsStOf {
  float* v;
  NtSt operator()(uint32_t stage) const { return NtSt{v + (size_t)stage * kNtsStageFloats}; }
};
struct RtEvalOf {
  const float* w;
  SearchEval operator()(const Board& b) const { return SearchEval{rt_q(rt_gather(w, b)), legal_mask(b)}; }
};
struct LtEvalOf {
  const float* w;
  SearchEval operator()(const Board& b) const { return SearchEval{lt_q(lt_gather(w, lt_indices(b))), legal_mask(b)}; }
};
struct AvEvalOf {
  const float* w;
  SearchEval operator()(const Board& b) const { const AvEval ev = av_eval(w, b); return SearchEval{av_row(ev), ev.c.legal}; }
};
struct NtEvalOf {
  const float* w;
  SearchEval operator()(const Board& b) const { const NtEval ev = nt_eval(b, NtLd{w}); return SearchEval{ev.q, ev.legal}; }
};
struct NtsEvalOf {
  const float* w;
  uint32_t stages;
  SearchEval operator()(const Board& b) const {
    const NtEval ev = nts_eval(b, stages, NtsLdOf{w});
    return SearchEval{ev.q, ev.legal};
  }
};
// the searched row of a board: DEPTH 1 = one level of expectimax over the spawn (search_row, the chance nodes evaluated
// serially), 2 = the two-level row (search_row2: the same serial walk one level further down)
template <int DEPTH, class Eval>
inline SearchEval search_eval(const Board& s, const Eval& eval) {
  if constexpr (DEPTH == 1) return search_row(s, [&](uint32_t, const Board& node) { return search_best_of(eval(node)); });
  else return search_row2(s, [&](const Board& x) { return search_best_of(eval(x)); });
}
// q2048_{av,nt,nts}_search_lookup*; the callers have checked the arguments
template <int DEPTH, class Eval>
int search_lookup_impl(Eval eval, const uint8_t* boards, int64_t B, float* q_out, uint8_t* legal_out) {
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const SearchEval ev = search_eval<DEPTH>(b, eval);
      q_out[4 * i] = ev.q.q0; q_out[4 * i + 1] = ev.q.q1; q_out[4 * i + 2] = ev.q.q2; q_out[4 * i + 3] = ev.q.q3;
      legal_out[i] = (uint8_t)ev.legal;
    }
  });
  return Q2048_OK;
}
// ---- the player on weights (q2048_{rt,lt,av,nt,nts}_play_rollout and the searched players): play_rollout_n's loop with
// the row and the legal-move mask of `row_of(board)`; the same play_action as the kernels, envs split over the threads,
// the weights only read.  The callers have checked the arguments.
template <class RowOf>
int play_loop(uint8_t* boards, q2048_aux* aux, int64_t B, int64_t steps, double eps, uint64_t seed, uint64_t env_id0,
              uint32_t ctr0, uint32_t flags, int64_t* stats_i, double* stats_f, RowOf row_of) {
  if (B == 0 || steps == 0) return Q2048_OK;
  const uint64_t eps_t = eps_threshold(eps);
  const ImageLuts lut{&g_lut_image};
  const int env = env_bits(flags);
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
    Stats& st = sp[tid];
    for (int64_t i = lo; i < hi; ++i) {
      const uint64_t id = env_id0 + (uint64_t)i;
      Board b;
      load_board(boards, i, b);
      Aux a = ld_aux(aux, i);
      const DrawPrep prep = draws_prepare(seed, id, kStreamStep);
      double reward_sum = 0.0;
      for (int64_t t = 0; t < steps; ++t) {
        const Draws x = draws_at(prep, ctr0 + (uint32_t)t);
        Draws y{0u, 0u, 0u, 0u};
        if (env & kEnvDqn) y = draws(seed, id, ctr0 + (uint32_t)t, kStreamOver);
        const SearchEval ev = row_of(b);
        bool explored;
        const int act = play_action(ev.legal, ev.q.q0, ev.q.q1, ev.q.q2, ev.q.q3, eps_t, x.x0, x.x1, explored);
        const StepOut o = env_step_any(env, b, a, act, x.x2, x.x3, y.x0, y.x1, lut);
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        reward_sum += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          begin_episode(b, a, seed, id, (env & kEnvResetShaping) != 0);
        }
      }
      st.i[Q2048_ST_STEPS] += (uint64_t)steps;
      st.f[Q2048_SF_REWARD] += reward_sum;
      store_board(boards, i, b);
      st_aux(aux, i, a);
    }
  });
  stats_merge(parts, used, stats_i, stats_f);
  return Q2048_OK;
}
// the searched player at a depth the caller has checked (1 or 2)
template <class Eval>
int search_play_impl(Eval eval, int depth, uint8_t* boards, q2048_aux* aux, int64_t B, int64_t steps, double eps,
                     uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t* stats_i, double* stats_f) {
  if (depth == 1)
    return play_loop(boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f,
                     [=](const Board& b) { return search_eval<1>(b, eval); });
  return play_loop(boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f,
                   [=](const Board& b) { return search_eval<2>(b, eval); });
}
template <class Eval>
int search_lookup_depth(Eval eval, int depth, const uint8_t* boards, int64_t B, float* q_out, uint8_t* legal_out) {
  return depth == 1 ? search_lookup_impl<1>(eval, boards, B, q_out, legal_out)
                    : search_lookup_impl<2>(eval, boards, B, q_out, legal_out);
}

// ---- bulk moves of rows into a table (import, merge, fold, unfold) ----------------------------------------------
// the one- or two-word key of a table, as the type the probes are compiled for: f(Geo<4>::Key) or f(Geo<5>::Key)
template <class F>
inline void with_key(int key_words, u64 k0, u64 k1, F&& f) {
  if (key_words == 1) f(Geo<4>::Key{k0});
  else f(Geo<5>::Key{k0, k1});
}

// The device's find-or-create-and-combine (combine_into, q2048_kernels.hip), value for value, for merge, fold and
// unfold: float32, the product rounded before the sum sees it (the volatile keeps a compiler that contracts by default
// from fusing the two).  Slots of `src` are split over the threads, every thread counts into its own Part, and the
// callers see to it that one thread alone brings a given key: one writer per dst row.
inline float mul_rn(float a, float b) { volatile float p = a * b; return p; }
inline float merge_value(int mode, float d, float s, float w, float one_minus_w) {
  if (mode == Q2048_MERGE_ADD) return d + mul_rn(w, s);
  if (mode == Q2048_MERGE_BLEND) { const float keep = mul_rn(one_minus_w, d); return keep + mul_rn(w, s); }
  return std::fabs(s) > std::fabs(d) ? s : d;
}
struct Part { uint64_t lead[2] = {0, 0}, created = 0, combined = 0, dropped = 0; uint32_t bits = 0; };   // lead: read, skipped
template <class Key>
inline void combine_into(q2048_slot* dst, u64 mask, const Key& key, const float q[4], int mode, float w, float one_minus_w,
                         Part& p) {
  bool inserted;
  const int64_t slot = probe_insert(dst, mask, key, key_home(key, mask), inserted, kMaxProbe);
  if (slot < 0) { ++p.dropped; p.bits |= Q2048_STATUS_TABLE_FULL; return; }
  if (inserted) {
    ++p.created;
    if (deep_row(key, mask, (u64)slot)) p.bits |= Q2048_STATUS_DEEP_ROW;
    for (int a = 0; a < 4; ++a) st_f32(&dst[slot].q[a], mode == Q2048_MERGE_ADD ? mul_rn(w, q[a]) : q[a]);
  } else {
    ++p.combined;
    for (int a = 0; a < 4; ++a) st_f32(&dst[slot].q[a], merge_value(mode, ld_f32(&dst[slot].q[a]), q[a], w, one_minus_w));
  }
}
// walk(lo, hi, part) over the slots [0, cap) of the source, split over the threads; then
// counters += {the first `lead` of part.lead, rows written (created + combined + dropped), created, combined, dropped}
template <class Walk>
inline void combine_ranges(int64_t cap, int lead, uint64_t* counters, uint32_t* status, Walk walk) {
  std::vector<Part> parts((size_t)threads_for(cap));
  Part* part = parts.data();
  const int used = parallel_ranges(cap, [=](int64_t lo, int64_t hi, int t) {
    Part p;
    walk(lo, hi, p);
    part[t] = p;
  });
  uint32_t bits = 0u;
  for (int t = 0; t < used; ++t) {
    const Part& p = parts[(size_t)t];
    for (int l = 0; l < lead; ++l) counters[l] += p.lead[l];
    counters[lead] += p.created + p.combined + p.dropped;
    counters[lead + 1] += p.created;
    counters[lead + 2] += p.combined;
    counters[lead + 3] += p.dropped;
    bits |= p.bits;
  }
  if (bits && status != nullptr) status_or(status, bits);
}
}  // namespace

extern "C" {

int q2048_abi_version(void) { return Q2048_ABI_VERSION; }

int q2048_claim_timeouts(uint64_t* count_host) {
  if (count_host == nullptr) return Q2048_ERR_NULL;
  *count_host = (uint64_t)__atomic_load_n(&g_claim_timeouts, __ATOMIC_RELAXED);
  return Q2048_OK;
}

const char* q2048_strerror(int code) { return error_text(code); }
size_t q2048_sizeof_aux(void) { return sizeof(q2048_aux); }
size_t q2048_sizeof_slot(void) { return sizeof(q2048_slot); }
size_t q2048_sizeof_rowcache(int n) { return n == 4 ? sizeof(RowCache<4>) : n == 5 ? sizeof(RowCache<5>) : 0; }
int q2048_rowcache_rebind(void* row_cache, int64_t B, int n, const q2048_slot* from_table, int from_cap_log2,
                          const q2048_slot* to_table, int to_cap_log2, void*) {
  if (int e = check_batch(B, n)) return e;
  if (int e = check_table(from_table, from_cap_log2)) return e;   // (an address of the past: never dereferenced)
  if (int e = check_table(to_table, to_cap_log2)) return e;
  if (row_cache == nullptr) return Q2048_ERR_NULL;
  if (!aligned16(row_cache)) return Q2048_ERR_ALIGN;
  const u64 tag_from = cache_tag(from_table, (1ull << from_cap_log2) - 1ull), tag_to = cache_tag(to_table, (1ull << to_cap_log2) - 1ull);
  if (n == 4) rowcache_rebind_n<4>(row_cache, B, tag_from, tag_to);
  else rowcache_rebind_n<5>(row_cache, B, tag_from, tag_to);
  return Q2048_OK;
}

int q2048_env_init(uint8_t* boards, q2048_aux* aux, int64_t B, int n, uint64_t seed, uint64_t env_id0, void*) {
  if (int e = check_batch(B, n)) return e;
  if (boards == nullptr || aux == nullptr) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux)) return Q2048_ERR_ALIGN;
  if (B == 0) return Q2048_OK;
  if (n == 4) env_init_impl<4>(boards, aux, B, seed, env_id0); else env_init_impl<5>(boards, aux, B, seed, env_id0);
  return Q2048_OK;
}
int q2048_env_reset_ex(uint8_t* boards, q2048_aux* aux, const uint8_t* mask, int64_t B, int n, uint64_t seed,
                       uint64_t env_id0, uint32_t flags, void*) {
  if (int e = check_batch(B, n)) return e;
  if (int e = check_flags(flags)) return e;
  if (boards == nullptr || aux == nullptr) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux)) return Q2048_ERR_ALIGN;
  if (B == 0) return Q2048_OK;
  if (n == 4) env_reset_impl<4>(boards, aux, mask, B, seed, env_id0, flags);
  else env_reset_impl<5>(boards, aux, mask, B, seed, env_id0, flags);
  return Q2048_OK;
}
int q2048_env_reset(uint8_t* boards, q2048_aux* aux, const uint8_t* mask, int64_t B, int n, uint64_t seed,
                    uint64_t env_id0, void* stream) {
  return q2048_env_reset_ex(boards, aux, mask, B, n, seed, env_id0, 0u, stream);
}
int q2048_env_step(uint8_t* boards, q2048_aux* aux, const uint8_t* actions, int64_t B, int n, uint64_t seed,
                   uint64_t env_id0, uint32_t ctr, float* reward, uint8_t* done, uint8_t* max_log2, uint32_t* status,
                   void*) {
  return env_step_impl(boards, boards, aux, actions, B, n, seed, env_id0, ctr, 0u, reward, done, max_log2, nullptr,
                       status, nullptr, nullptr, nullptr, nullptr, 1);
}
int q2048_env_step_ex(uint8_t* boards, q2048_aux* aux, const uint8_t* actions, int64_t B, int n, uint64_t seed,
                      uint64_t env_id0, uint32_t ctr, uint32_t flags, const uint32_t* draws4, float* reward,
                      uint8_t* done, uint8_t* max_log2, uint32_t* status, void*) {
  if (draws4 == nullptr)
    return env_step_impl(boards, boards, aux, actions, B, n, seed, env_id0, ctr, flags, reward, done, max_log2,
                         nullptr, status, nullptr, nullptr, nullptr, nullptr, 1);
  return env_step_impl(boards, boards, aux, actions, B, n, 0, 0, 0, flags, reward, done, max_log2, nullptr, status,
                       draws4, draws4 + 1, draws4 + 2, draws4 + 3, 4);
}
int q2048_env_step_to(const uint8_t* boards_in, uint8_t* boards_out, q2048_aux* aux, const uint8_t* actions, int64_t B,
                      int n, uint64_t seed, uint64_t env_id0, uint32_t ctr, uint32_t flags, float* reward,
                      uint8_t* done, uint8_t* max_log2, int32_t* max_tile, uint32_t* status, void*) {
  return env_step_impl(boards_in, boards_out, aux, actions, B, n, seed, env_id0, ctr, flags, reward, done, max_log2,
                       max_tile, status, nullptr, nullptr, nullptr, nullptr, 1);
}
int q2048_env_step_draws(uint8_t* boards, q2048_aux* aux, const uint8_t* actions, const uint32_t* draw_pos,
                         const uint32_t* draw_val, int64_t B, int n, float* reward, uint8_t* done, uint8_t* max_log2,
                         uint32_t* status, void*) {
  if (!draw_pos || !draw_val) return Q2048_ERR_NULL;
  return env_step_impl(boards, boards, aux, actions, B, n, 0, 0, 0, 0u, reward, done, max_log2, nullptr, status,
                       draw_pos, draw_val, nullptr, nullptr, 1);
}

int q2048_q_choose(const q2048_slot* table, int cap_log2, const uint8_t* boards, int64_t B, int n, double eps,
                   uint64_t seed, uint64_t env_id0, uint32_t ctr, uint32_t flags, uint8_t* actions, uint32_t* status,
                   void*) {
  return q_choose_impl(table, cap_log2, boards, B, n, eps, seed, env_id0, ctr, flags, nullptr, actions, status,
                       nullptr, nullptr);
}
int q2048_q_choose_cached(const q2048_slot* table, int cap_log2, const uint8_t* boards, int64_t B, int n, double eps,
                          uint64_t seed, uint64_t env_id0, uint32_t ctr, uint32_t flags, const void* row_cache,
                          uint8_t* actions, uint32_t* status, void*) {
  return q_choose_impl(table, cap_log2, boards, B, n, eps, seed, env_id0, ctr, flags, row_cache, actions, status,
                       nullptr, nullptr);
}
int q2048_q_choose_draws(const q2048_slot* table, int cap_log2, const uint8_t* boards, const uint32_t* draw_eps,
                         const uint32_t* draw_act, int64_t B, int n, double eps, uint64_t env_id0, uint32_t flags,
                         uint8_t* actions, uint32_t* status, void*) {
  if (!draw_eps || !draw_act) return Q2048_ERR_NULL;
  return q_choose_impl(table, cap_log2, boards, B, n, eps, 0, env_id0, 0, flags, nullptr, actions, status, draw_eps,
                       draw_act);
}
int q2048_q_update_cached(q2048_slot* table, int cap_log2, const uint8_t* boards_s, const uint8_t* actions,
                          const float* reward, const uint8_t* boards_s2, const uint8_t* done, int64_t B, int n,
                          double lr, double gamma, uint64_t env_id0, uint32_t flags, void* row_cache,
                          int64_t* stats_i, uint32_t* status, void*) {
  if (int e = check_batch(B, n)) return e;
  if (int e = check_flags(flags)) return e;
  if (int e = check_table(table, cap_log2)) return e;
  if (!boards_s || !actions || !reward || !boards_s2 || !done || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards_s) || !aligned16(boards_s2) || !aligned16(row_cache)) return Q2048_ERR_ALIGN;
  if (!(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  if (B == 0) return Q2048_OK;
  const u64 mask = (1ull << cap_log2) - 1ull;
  if (n == 4) q_update_impl_n<4>(table, mask, boards_s, actions, reward, boards_s2, done, B, lr, gamma, env_id0, flags, stats_i, status, row_cache);
  else q_update_impl_n<5>(table, mask, boards_s, actions, reward, boards_s2, done, B, lr, gamma, env_id0, flags, stats_i, status, row_cache);
  return Q2048_OK;
}
int q2048_q_update(q2048_slot* table, int cap_log2, const uint8_t* boards_s, const uint8_t* actions,
                   const float* reward, const uint8_t* boards_s2, const uint8_t* done, int64_t B, int n, double lr,
                   double gamma, uint64_t env_id0, uint32_t flags, int64_t* stats_i, uint32_t* status, void* stream) {
  return q2048_q_update_cached(table, cap_log2, boards_s, actions, reward, boards_s2, done, B, n, lr, gamma, env_id0,
                               flags, nullptr, stats_i, status, stream);
}
int q2048_q_lookup(const q2048_slot* table, int cap_log2, const uint8_t* boards, int64_t B, int n, uint64_t env_id0,
                   uint32_t flags, float* q_out, uint8_t* found, uint32_t* status, void*) {
  if (int e = check_batch(B, n)) return e;
  if (int e = check_flags(flags, 0u, Q2048_FLAG_SYMMETRIC)) return e;
  if (n == 5 && (flags & Q2048_FLAG_SYMMETRIC)) return Q2048_ERR_UNSUPPORTED;
  if (int e = check_table(table, cap_log2)) return e;
  if (!boards || !q_out || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(q_out)) return Q2048_ERR_ALIGN;
  if (B == 0) return Q2048_OK;
  const u64 mask = (1ull << cap_log2) - 1ull;
  if (n == 4) q_lookup_impl_n<4>(table, mask, boards, B, env_id0, flags, q_out, found, status);
  else q_lookup_impl_n<5>(table, mask, boards, B, env_id0, flags, q_out, found, status);
  return Q2048_OK;
}

int q2048_fused_rollout_opts(uint8_t* boards, q2048_aux* aux, q2048_slot* table, int cap_log2, int64_t B, int n,
                             int64_t steps, double eps, double lr, double gamma, uint64_t seed, uint64_t env_id0,
                             uint32_t ctr0, uint32_t flags, int64_t* stats_i, double* stats_f, uint32_t* status,
                             const q2048_rollout_opts* opts, void*) {
  q2048_rollout_opts o = {};
  if (opts != nullptr) {
    // the 56-byte layout shipped before `line_summary` (no side array) or this one
    if (opts->size != sizeof(q2048_rollout_opts) && opts->size != offsetof(q2048_rollout_opts, line_summary)) return Q2048_ERR_SIZE;
    std::memcpy(&o, opts, opts->size);
  }
  if (int e = check_batch(B, n)) return e;
  if (int e = check_flags(flags, 0u, Q2048_FLAG_SYMMETRIC)) return e;
  if (n == 5 && (flags & Q2048_FLAG_SYMMETRIC)) return Q2048_ERR_UNSUPPORTED;
  if (o.log != nullptr && (o.log_count == nullptr || o.log_capacity < 0)) return Q2048_ERR_NULL;
  if (o.log != nullptr && !aligned16(o.log)) return Q2048_ERR_ALIGN;
  if (o.row_cache != nullptr && !aligned16(o.row_cache)) return Q2048_ERR_ALIGN;
  if (reinterpret_cast<uintptr_t>(o.line_summary) & 7u) return Q2048_ERR_ALIGN;
  if (o.stats_mirror != nullptr && (o.mirror_ticket == nullptr || stats_i == nullptr || stats_f == nullptr))
    return Q2048_ERR_NULL;
  if (o.stats_mirror != nullptr && (reinterpret_cast<uintptr_t>(o.stats_mirror) & 7u)) return Q2048_ERR_ALIGN;
  if (int e = check_table(table, cap_log2)) return e;
  if (!boards || !aux || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux)) return Q2048_ERR_ALIGN;
  if (steps < 0 || steps > (1 << 30)) return Q2048_ERR_SIZE;
  if (!(eps >= 0.0 && eps <= 1.0) || !(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  if (B == 0 || steps == 0) return Q2048_OK;
  const u64 mask = (1ull << cap_log2) - 1ull;
  if (n == 4) fused_rollout_n<4>(boards, aux, table, mask, B, (int)steps, eps, lr, gamma, seed, env_id0, ctr0, flags,
                                 stats_i, stats_f, status, o.log, o.log_capacity, o.log_count, o.row_cache, nullptr);
  else fused_rollout_n<5>(boards, aux, table, mask, B, (int)steps, eps, lr, gamma, seed, env_id0, ctr0, flags, stats_i,
                          stats_f, status, o.log, o.log_capacity, o.log_count, o.row_cache, o.line_summary);
  if (o.stats_mirror != nullptr) {               // the statistics as they stand after this call, and its number
    uint64_t* m = static_cast<uint64_t*>(o.stats_mirror);
    std::memcpy(m, stats_i, sizeof(int64_t) * Q2048_NSTAT_I);
    std::memcpy(m + Q2048_NSTAT_I, stats_f, sizeof(double) * Q2048_NSTAT_F);
    m[Q2048_MIRROR_SEQ] = ++o.mirror_ticket[1];
  }
  return Q2048_OK;
}
int q2048_play_rollout(uint8_t* boards, q2048_aux* aux, const q2048_slot* table, int cap_log2, int64_t B, int n,
                       int64_t steps, double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                       int64_t* stats_i, double* stats_f, uint32_t* status, void*) {
  if (int e = check_batch(B, n)) return e;
  if (int e = check_flags(flags, kAbiFlags & ~(Q2048_FLAG_INDEPENDENT | Q2048_FLAG_ENV_DQN | Q2048_FLAG_RESET_SHAPING),
                          Q2048_FLAG_SYMMETRIC))
    return e;
  if (n == 5 && (flags & Q2048_FLAG_SYMMETRIC)) return Q2048_ERR_UNSUPPORTED;
  if (int e = check_table(table, cap_log2)) return e;
  if (!boards || !aux || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux)) return Q2048_ERR_ALIGN;
  if (steps < 0 || steps > (1 << 30)) return Q2048_ERR_SIZE;
  if (!(eps >= 0.0 && eps <= 1.0)) return Q2048_ERR_RANGE;
  if (B == 0 || steps == 0) return Q2048_OK;
  const u64 mask = (1ull << cap_log2) - 1ull;
  if (n == 4) play_rollout_n<4>(boards, aux, table, mask, B, (int)steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f, status);
  else play_rollout_n<5>(boards, aux, table, mask, B, (int)steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f, status);
  return Q2048_OK;
}
int q2048_fused_rollout(uint8_t* boards, q2048_aux* aux, q2048_slot* table, int cap_log2, int64_t B, int n,
                        int64_t steps, double eps, double lr, double gamma, uint64_t seed, uint64_t env_id0,
                        uint32_t ctr0, uint32_t flags, int64_t* stats_i, double* stats_f, uint32_t* status,
                        void* stream) {
  return q2048_fused_rollout_opts(boards, aux, table, cap_log2, B, n, steps, eps, lr, gamma, seed, env_id0, ctr0,
                                  flags, stats_i, stats_f, status, nullptr, stream);
}
int q2048_fused_rollout_log(uint8_t* boards, q2048_aux* aux, q2048_slot* table, int cap_log2, int64_t B, int n,
                            int64_t steps, double eps, double lr, double gamma, uint64_t seed, uint64_t env_id0,
                            uint32_t ctr0, uint32_t flags, int64_t* stats_i, double* stats_f, uint32_t* status,
                            q2048_episode* log, int64_t log_capacity, uint64_t* log_count, void* stream) {
  q2048_rollout_opts o = {};
  o.size = (uint32_t)sizeof(o);
  o.log = log; o.log_capacity = log_capacity; o.log_count = log_count;
  return q2048_fused_rollout_opts(boards, aux, table, cap_log2, B, n, steps, eps, lr, gamma, seed, env_id0, ctr0,
                                  flags, stats_i, stats_f, status, &o, stream);
}

int64_t q2048_det_workspace_bytes(int64_t B, int cap_log2) {
  if (B < 0 || B > 0x7fffffffll || cap_log2 < 4 || cap_log2 > 40) return Q2048_ERR_SIZE;
  return 256;                                     // the host step keeps its scratch itself
}
int q2048_det_rollout(uint8_t* boards, q2048_aux* aux, q2048_slot* table, int cap_log2, int64_t B, int n,
                      int64_t steps, double eps, double lr, double gamma, uint64_t seed, uint64_t env_id0,
                      uint32_t ctr0, uint32_t flags, int64_t* stats_i, double* stats_f, uint32_t* status,
                      void* workspace, int64_t workspace_bytes, void* stream) {
  return q2048_det_rollout_cached(boards, aux, table, cap_log2, B, n, steps, eps, lr, gamma, seed, env_id0, ctr0, flags,
                                  stats_i, stats_f, status, workspace, workspace_bytes, nullptr, stream);
}
int q2048_det_rollout_cached(uint8_t* boards, q2048_aux* aux, q2048_slot* table, int cap_log2, int64_t B, int n,
                             int64_t steps, double eps, double lr, double gamma, uint64_t seed, uint64_t env_id0,
                             uint32_t ctr0, uint32_t flags, int64_t* stats_i, double* stats_f, uint32_t* status,
                             void* workspace, int64_t workspace_bytes, void* row_cache, void*) {
  if (int e = check_batch(B, n)) return e;
  if (row_cache != nullptr && !aligned16(row_cache)) return Q2048_ERR_ALIGN;
  if (int e = check_flags(flags, Q2048_FLAG_NO_LEARN | Q2048_FLAG_PLAY_ONLY)) return e;
  if (B > 0x7fffffffll) return Q2048_ERR_SIZE;
  if (int e = check_table(table, cap_log2)) return e;
  if (!boards || !aux || !status || !workspace) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux) || (reinterpret_cast<uintptr_t>(workspace) & 255u)) return Q2048_ERR_ALIGN;
  if (steps < 0 || steps > (1 << 30) || workspace_bytes < 256) return Q2048_ERR_SIZE;
  if (!(eps >= 0.0 && eps <= 1.0) || !(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  if (B == 0 || steps == 0) return Q2048_OK;
  const u64 mask = (1ull << cap_log2) - 1ull;
  if (n == 4) det_rollout_n<4>(boards, aux, table, mask, B, steps, eps, lr, gamma, seed, env_id0, ctr0, flags, stats_i, stats_f, status, row_cache);
  else det_rollout_n<5>(boards, aux, table, mask, B, steps, eps, lr, gamma, seed, env_id0, ctr0, flags, stats_i, stats_f, status, row_cache);
  return Q2048_OK;
}

// the chunked DEVICE allocator has no host form: host tables are the caller's plain memory
int q2048_table_alloc(int, size_t, q2048_slot** out) { if (out) *out = nullptr; return Q2048_ERR_UNSUPPORTED; }
int q2048_table_reserve(int, int, size_t, q2048_slot** out) { if (out) *out = nullptr; return Q2048_ERR_UNSUPPORTED; }
int q2048_table_grow_begin(q2048_slot*, int, int, q2048_growth** out) { if (out) *out = nullptr; return Q2048_ERR_UNSUPPORTED; }
int q2048_table_grow_poll(q2048_growth*) { return Q2048_ERR_UNSUPPORTED; }
int q2048_table_grow_wait(q2048_growth*, double*) { return Q2048_ERR_UNSUPPORTED; }
int q2048_table_grow_commit(q2048_growth*, int, uint32_t, q2048_slot** out, void*) { if (out) *out = nullptr; return Q2048_ERR_UNSUPPORTED; }
int q2048_table_grow_finish(q2048_growth*, int64_t*) { return Q2048_ERR_UNSUPPORTED; }
int q2048_table_grow_abort(q2048_growth*) { return Q2048_ERR_UNSUPPORTED; }
int q2048_table_grow(q2048_slot*, int, int, int, q2048_slot** out, int64_t*, void*) { if (out) *out = nullptr; return Q2048_ERR_UNSUPPORTED; }
int q2048_table_trim(q2048_slot*) { return Q2048_ERR_UNSUPPORTED; }
int q2048_table_free(q2048_slot* table) { return table == nullptr ? Q2048_OK : Q2048_ERR_UNSUPPORTED; }

int q2048_table_probe(q2048_slot* table, int cap_log2, int64_t lanes, int steps, uint64_t, void*) {
  if (int e = check_table(table, cap_log2)) return e;
  if (lanes < 0 || lanes > ((int64_t)1 << 30) || steps < 0 || steps > (1 << 16)) return Q2048_ERR_SIZE;
  return Q2048_OK;                                // placement is a property of device memory: nothing to probe here
}

int q2048_table_export(const q2048_slot* table, int cap_log2, uint64_t* keys_out, float* q_out, int64_t max_rows,
                       int key_words, int64_t* count, void*) {
  if (int e = check_table(table, cap_log2)) return e;
  if (count == nullptr) return Q2048_ERR_NULL;
  if ((keys_out == nullptr) != (q_out == nullptr) || max_rows < 0) return Q2048_ERR_SIZE;
  if (key_words != 1 && key_words != 2) return Q2048_ERR_SIZE;
  if (q_out != nullptr && !aligned16(q_out)) return Q2048_ERR_ALIGN;
  const u64 cap = 1ull << cap_log2;
  int64_t at = *count;                            // adds to *count, as the device does
  for (u64 i = 0; i < cap; ++i) {
    if (table[i].key == 0ull) continue;
    if (keys_out != nullptr && at < max_rows) {
      keys_out[at * key_words] = table[i].key;
      if (key_words == 2) keys_out[at * 2 + 1] = table[i].reserved;
      std::memcpy(q_out + 4 * at, table[i].q, 16);
    }
    ++at;
  }
  *count = at;
  return Q2048_OK;
}
// the device's line summaries, byte for byte (q2048_kernels.hip: summary_fp, k_table_summarise): four 16-bit
// fingerprints per 128-byte line, 0 = empty, the same word in the `reserved` field of the line's four slots
int q2048_table_summarise(q2048_slot* table, int cap_log2, void*) {
  if (int e = check_table(table, cap_log2)) return e;
  const int64_t lines = (int64_t)((1ull << cap_log2) >> 2);
  parallel_ranges(lines, [=](int64_t lo, int64_t hi, int) {
    for (int64_t l = lo; l < hi; ++l) {
      q2048_slot* s = table + (l << 2);
      u64 sum = 0ull;
      for (int r = 0; r < 4; ++r)
        if (s[r].key != 0ull) sum |= (((mix64(s[r].key) >> 48) & 0xffffull) | 1ull) << (16 * r);
      for (int r = 0; r < 4; ++r) s[r].reserved = sum;
    }
  });
  return Q2048_OK;
}
// the device's side array, byte for byte (k_table_summarise_side): the same words beside the table, which is only read
int q2048_table_summarise_side(const q2048_slot* table, int cap_log2, int key_words, uint64_t* summary, void*) {
  if (table == nullptr || summary == nullptr) return Q2048_ERR_NULL;
  if (key_words != 1 && key_words != 2) return Q2048_ERR_SIZE;
  if (reinterpret_cast<uintptr_t>(summary) & 7u) return Q2048_ERR_ALIGN;
  if (int e = check_table(table, cap_log2)) return e;
  const int64_t lines = (int64_t)((1ull << cap_log2) >> 2);
  parallel_ranges(lines, [=](int64_t lo, int64_t hi, int) {
    for (int64_t l = lo; l < hi; ++l) {
      const q2048_slot* s = table + (l << 2);
      u64 sum = 0ull;
      for (int r = 0; r < 4; ++r) {
        const u64 k = s[r].key;
        if (k == 0ull) continue;
        const u64 hash = key_words == 2 ? key_hash(Geo<5>::Key{k, (u64)s[r].reserved}) : key_hash(Geo<4>::Key{k});
        sum |= summary_fp(hash) << (16 * r);
      }
      summary[l] = sum;
    }
  });
  return Q2048_OK;
}
int q2048_table_count(const q2048_slot* table, int cap_log2, int64_t* count, void* stream) {
  return q2048_table_export(table, cap_log2, nullptr, nullptr, 0, 1, count, stream);
}
int q2048_table_import(q2048_slot* table, int cap_log2, const uint64_t* keys, const float* q, int64_t rows,
                       int key_words, uint32_t* status, void*) {
  if (int e = check_table(table, cap_log2)) return e;
  if (!keys || !q || !status) return Q2048_ERR_NULL;
  if (rows < 0 || (key_words != 1 && key_words != 2)) return Q2048_ERR_SIZE;
  if (!aligned16(q)) return Q2048_ERR_ALIGN;
  const u64 mask = (1ull << cap_log2) - 1ull;
  parallel_ranges(rows, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i)
      with_key(key_words, keys[key_words * i], key_words == 2 ? keys[2 * i + 1] : 0ull, [&](const auto& key) {
        bool inserted;
        const int64_t slot = probe_insert(table, mask, key, key_home(key, mask), inserted, kMaxProbe);
        if (slot < 0) { status_or(status, Q2048_STATUS_TABLE_FULL); return; }
        if (deep_row(key, mask, (u64)slot)) status_or(status, Q2048_STATUS_DEEP_ROW);
        for (int a = 0; a < 4; ++a) st_f32(&table[slot].q[a], q[4 * i + a]);
      });
  });
  return Q2048_OK;
}

// the device's merge (k_table_merge): every occupied row of `src` (rows read == rows written: no leading counter)
int q2048_table_merge(q2048_slot* dst, int dst_cap_log2, const q2048_slot* src, int src_cap_log2, int key_words,
                      int mode, float w, uint64_t* counters, uint32_t* status, void*) {
  if (int e = check_merge(dst, dst_cap_log2, src, src_cap_log2, counters, key_words == 1 || key_words == 2, true, mode, w)) return e;
  const u64 mask = (1ull << dst_cap_log2) - 1ull;
  const float one_minus_w = 1.0f - w;
  combine_ranges((int64_t)1 << src_cap_log2, 0, counters, status, [=](int64_t lo, int64_t hi, Part& p) {
    for (int64_t i = lo; i < hi; ++i) {
      const q2048_slot& s = src[i];
      if (s.key == 0ull) continue;
      with_key(key_words, s.key, s.reserved, [&](const auto& key) { combine_into(dst, mask, key, s.q, mode, w, one_minus_w, p); });
    }
  });
  return Q2048_OK;
}

// the device's fold (k_table_fold): the same walk of the orbit (fold_orbit, q2048_core.hpp), the leader's one
// combine_into; leads with rows read
namespace {
static_assert(Q2048_FOLD_MEAN == kFoldMean && Q2048_FOLD_MEAN_TRAINED == kFoldMeanTrained && Q2048_FOLD_SUM == kFoldSum &&
              Q2048_FOLD_MAXABS == kFoldMaxAbs, "q2048.h / q2048_core.hpp");
}  // namespace
int q2048_table_fold(q2048_slot* dst, int dst_cap_log2, const q2048_slot* src, int src_cap_log2, int key_words, int fold,
                     int mode, float w, uint64_t* counters, uint32_t* status, void*) {
  if (!dst || !src || !counters) return Q2048_ERR_NULL;
  if (key_words == 2) return Q2048_ERR_UNSUPPORTED;
  const bool fold_ok = fold == Q2048_FOLD_MEAN || fold == Q2048_FOLD_MEAN_TRAINED || fold == Q2048_FOLD_SUM || fold == Q2048_FOLD_MAXABS;
  if (int e = check_merge(dst, dst_cap_log2, src, src_cap_log2, counters, key_words == 1, fold_ok, mode, w)) return e;
  const u64 mask = (1ull << dst_cap_log2) - 1ull, src_mask = (1ull << src_cap_log2) - 1ull;
  const float one_minus_w = 1.0f - w;
  combine_ranges((int64_t)1 << src_cap_log2, 1, counters, status, [=](int64_t lo, int64_t hi, Part& p) {
    const auto find = [src, src_mask](uint64_t k, float out[4]) {
      Row row;
      const bool present = probe_find(src, src_mask, Geo<4>::Key{(u64)k}, row, kMaxProbe) >= 0;
      out[0] = row.q0; out[1] = row.q1; out[2] = row.q2; out[3] = row.q3;
      return present;
    };
    for (int64_t i = lo; i < hi; ++i) {
      const q2048_slot& s = src[i];
      if (s.key == 0ull) continue;
      ++p.lead[0];
      uint64_t canon;
      float r[4];
      const bool leads = fold == Q2048_FOLD_MEAN           ? fold_orbit<kFoldMean>(s.key, s.q, find, canon, r)
                         : fold == Q2048_FOLD_MEAN_TRAINED ? fold_orbit<kFoldMeanTrained>(s.key, s.q, find, canon, r)
                         : fold == Q2048_FOLD_SUM          ? fold_orbit<kFoldSum>(s.key, s.q, find, canon, r)
                                                           : fold_orbit<kFoldMaxAbs>(s.key, s.q, find, canon, r);
      if (!leads) continue;                                  // another row leads this orbit
      combine_into(dst, mask, Geo<4>::Key{(u64)canon}, r, mode, w, one_minus_w, p);
    }
  });
  return Q2048_OK;
}

// the device's unfold (k_table_unfold): the same walk of the orbit (unfold_orbit, q2048_core.hpp), one combine_into
// per member (a source row's whole orbit is written by the thread that read the row, and orbits of distinct
// canonical keys are disjoint); leads with rows read, rows skipped
int q2048_table_unfold(q2048_slot* dst, int dst_cap_log2, const q2048_slot* src, int src_cap_log2, int key_words, int mode,
                       float w, uint64_t* counters, uint32_t* status, void*) {
  if (!dst || !src || !counters) return Q2048_ERR_NULL;
  if (key_words == 2) return Q2048_ERR_UNSUPPORTED;
  if (int e = check_merge(dst, dst_cap_log2, src, src_cap_log2, counters, key_words == 1, true, mode, w)) return e;
  const u64 mask = (1ull << dst_cap_log2) - 1ull;
  const float one_minus_w = 1.0f - w;
  combine_ranges((int64_t)1 << src_cap_log2, 2, counters, status, [=](int64_t lo, int64_t hi, Part& p) {
    const auto emit = [&p, dst, mask, mode, w, one_minus_w](uint64_t m, const Row& r) {
      const float q[4] = {r.q0, r.q1, r.q2, r.q3};
      combine_into(dst, mask, Geo<4>::Key{(u64)m}, q, mode, w, one_minus_w, p);
    };
    for (int64_t i = lo; i < hi; ++i) {
      const q2048_slot& s = src[i];
      if (s.key == 0ull) continue;
      ++p.lead[0];
      if (unfold_orbit(s.key, Row{s.q[0], s.q[1], s.q[2], s.q[3]}, emit) == 0u) ++p.lead[1];
    }
  });
  return Q2048_OK;
}

int q2048_canonicalize(const uint8_t* boards, int64_t B, int n, uint8_t* boards_out, uint8_t* sym_out, void*) {
  if (int e = check_batch(B, n)) return e;
  if (n != 4) return Q2048_ERR_UNSUPPORTED;
  if (boards == nullptr) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(boards_out)) return Q2048_ERR_ALIGN;
  if (B == 0) return Q2048_OK;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      bool ov;
      const uint32_t g = canonical_key(pack_key(b, ov)).g;
      if (boards_out != nullptr) store_board(boards_out, i, board_image(b, g));
      if (sym_out != nullptr) sym_out[i] = (uint8_t)g;
    }
  });
  return Q2048_OK;
}

int q2048_legal_moves(const uint8_t* boards, int64_t B, int n, uint8_t* mask_out, void*) {
  if (int e = check_batch(B, n)) return e;
  if (!boards || !mask_out) return Q2048_ERR_NULL;
  if (!aligned16(boards)) return Q2048_ERR_ALIGN;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      uint32_t m = 0, score;
      if (n == 4) { Board b; load_board(boards, i, b); for (int a = 0; a < 4; ++a) { Board t = b; m |= (uint32_t)move(t, a, score) << a; } }
      else { Board5 b; load_board(boards, i, b); for (int a = 0; a < 4; ++a) { Board5 t = b; m |= (uint32_t)move(t, a, score) << a; } }
      mask_out[i] = (uint8_t)m;
    }
  });
  return Q2048_OK;
}
int q2048_encode_onehot(const uint8_t* boards, int64_t B, int dtype, void* out, void*) {
  if (int e = check_batch(B, 4)) return e;
  if (B > (int64_t)0x7fffffff * 4) return Q2048_ERR_SIZE;            // the device's limit (64 threads per board)
  if (!boards || !out) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(out)) return Q2048_ERR_ALIGN;
  if (dtype != 0 && dtype != 1) return Q2048_ERR_RANGE;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t b = lo; b < hi; ++b)
      for (int c = 0; c < 16; ++c)
        for (int cell = 0; cell < 16; ++cell) {
          const bool hit = boards[16 * b + cell] == c;       // out[b][c][r][col], cell = 4 r + col
          if (dtype == 0) static_cast<float*>(out)[(b * 16 + c) * 16 + cell] = hit ? 1.f : 0.f;
          else static_cast<uint16_t*>(out)[(b * 16 + c) * 16 + cell] = hit ? 0x3F80u : 0u;
        }
  });
  return Q2048_OK;
}

int q2048_rt_choose(const float* weights, const uint8_t* boards, int64_t B, double eps, uint64_t seed, uint64_t env_id0,
                    uint32_t ctr, uint8_t* actions, void*) {
  if (int e = check_batch(B, 4)) return e;
  if (!weights || !boards || !actions) return Q2048_ERR_NULL;
  if (!aligned16(weights) || !aligned16(boards)) return Q2048_ERR_ALIGN;
  if (!(eps >= 0.0 && eps <= 1.0)) return Q2048_ERR_RANGE;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const Draws x = draws(seed, env_id0 + (uint64_t)i, ctr, kStreamStep);
      int act;
      if (draw_uniform(x.x0) < eps) act = draw_action(x.x1);
      else { const Row q = rt_q(rt_gather(weights, b)); act = argmax4(q.q0, q.q1, q.q2, q.q3); }
      actions[i] = (uint8_t)act;
    }
  });
  return Q2048_OK;
}
int q2048_rt_lookup(const float* weights, const uint8_t* boards, int64_t B, float* q_out, void*) {
  if (int e = check_batch(B, 4)) return e;
  if (!weights || !boards || !q_out) return Q2048_ERR_NULL;
  if (!aligned16(weights) || !aligned16(boards) || !aligned16(q_out)) return Q2048_ERR_ALIGN;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const Row q = rt_q(rt_gather(weights, b));
      q_out[4 * i] = q.q0; q_out[4 * i + 1] = q.q1; q_out[4 * i + 2] = q.q2; q_out[4 * i + 3] = q.q3;
    }
  });
  return Q2048_OK;
}
int q2048_rt_update(float* weights, const uint8_t* boards_s, const uint8_t* actions, const float* reward,
                    const uint8_t* boards_s2, const uint8_t* done, int64_t B, double lr, double gamma, uint32_t* status,
                    void*) {
  if (int e = check_batch(B, 4)) return e;
  if (!weights || !boards_s || !actions || !reward || !boards_s2 || !done || !status) return Q2048_ERR_NULL;
  if (!aligned16(weights) || !aligned16(boards_s) || !aligned16(boards_s2)) return Q2048_ERR_ALIGN;
  if (!(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      const int act = actions[i];
      if (act > 3) { status_or(status, Q2048_STATUS_BAD_ACTION); continue; }
      Board b_s, b_n;
      load_board(boards_s, i, b_s);
      load_board(boards_s2, i, b_n);
      const Row qn = rt_q(rt_gather(weights, b_n));
      const RtRows es = rt_gather(weights, b_s);
      const float d = rt_delta(row_get(rt_q(es), act), reward[i], max4(qn.q0, qn.q1, qn.q2, qn.q3), done[i] != 0, lr, gamma);
      rt_scatter(weights, b_s, es, act, d);
    }
  });
  return Q2048_OK;
}
int q2048_rt_fused_rollout(uint8_t* boards, q2048_aux* aux, float* weights, int64_t B, int64_t steps, double eps,
                           double lr, double gamma, uint64_t seed, uint64_t env_id0, uint32_t ctr0, int64_t* stats_i,
                           double* stats_f, uint32_t* status, void*) {
  if (int e = check_batch(B, 4)) return e;
  if (!boards || !aux || !weights || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux) || !aligned16(weights)) return Q2048_ERR_ALIGN;
  if (steps < 0 || steps > (1 << 30)) return Q2048_ERR_SIZE;
  if (!(eps >= 0.0 && eps <= 1.0) || !(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  if (B == 0 || steps == 0) return Q2048_OK;
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
    Stats& st = sp[tid];
    for (int64_t i = lo; i < hi; ++i) {
      const uint64_t id = env_id0 + (uint64_t)i;
      Board b;
      load_board(boards, i, b);
      Aux a = ld_aux(aux, i);
      double reward_sum = 0.0;
      RtRows es = rt_gather(weights, b);
      for (int64_t t = 0; t < steps; ++t) {
        const Draws x = draws(seed, id, ctr0 + (uint32_t)t, kStreamStep);
        const Board s = b;
        const Row q = rt_q(es);
        bool explored;
        const int act = eps_greedy(eps, x.x0, x.x1, q.q0, q.q1, q.q2, q.q3, explored);
        const StepOut o = env_step(b, a, act, x.x2, x.x3);
        RtRows en = rt_gather(weights, b);
        const Row qn = rt_q(en);
        const float d = rt_delta(row_get(q, act), o.reward, max4(qn.q0, qn.q1, qn.q2, qn.q3), o.done != 0, lr, gamma);
        rt_scatter(weights, s, es, act, d);
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        reward_sum += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          begin_episode(b, a, seed, id);
          es = rt_gather(weights, b);
        } else {
          const uint32_t ib[4] = {pack_row(b.r0), pack_row(b.r1), pack_row(b.r2), pack_row(b.r3)};
          const uint32_t is[4] = {pack_row(s.r0), pack_row(s.r1), pack_row(s.r2), pack_row(s.r3)};
          for (int r = 0; r < 4; ++r)
            if (ib[r] == is[r]) row_set(en.e[r], act, row_get(es.e[r], act) + d);
          es = en;
        }
      }
      st.i[Q2048_ST_STEPS] += (uint64_t)steps;
      st.f[Q2048_SF_REWARD] += reward_sum;
      store_board(boards, i, b);
      st_aux(aux, i, a);
    }
  });
  stats_merge(parts, used, stats_i, stats_f);
  return Q2048_OK;
}
// the greedy player on weights: play_loop with q2048_rt_lookup's row (RtEvalOf: rt_q of rt_gather)
int q2048_rt_play_rollout(uint8_t* boards, q2048_aux* aux, const float* weights, int64_t B, int64_t steps, double eps,
                          uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t* stats_i,
                          double* stats_f, uint32_t* status, void*) {
  if (int e = check_rt_play(boards, aux, weights, B, steps, eps, flags, status)) return e;
  return play_loop(boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f, RtEvalOf{weights});
}

// ---- the line-tuple family: the row-tuple functions above with lt_gather / lt_q / lt_scatter ----
int q2048_lt_choose(const float* weights, const uint8_t* boards, int64_t B, double eps, uint64_t seed, uint64_t env_id0,
                    uint32_t ctr, uint8_t* actions, void*) {
  if (int e = check_lt_choose(weights, boards, B, eps, actions)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const Draws x = draws(seed, env_id0 + (uint64_t)i, ctr, kStreamStep);
      int act;
      if (draw_uniform(x.x0) < eps) act = draw_action(x.x1);
      else { const Row q = lt_q(lt_gather(weights, lt_indices(b))); act = argmax4(q.q0, q.q1, q.q2, q.q3); }
      actions[i] = (uint8_t)act;
    }
  });
  return Q2048_OK;
}
int q2048_lt_lookup(const float* weights, const uint8_t* boards, int64_t B, float* q_out, void*) {
  if (int e = check_lt_lookup(weights, boards, B, q_out)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const Row q = lt_q(lt_gather(weights, lt_indices(b)));
      q_out[4 * i] = q.q0; q_out[4 * i + 1] = q.q1; q_out[4 * i + 2] = q.q2; q_out[4 * i + 3] = q.q3;
    }
  });
  return Q2048_OK;
}
int q2048_lt_update(float* weights, const uint8_t* boards_s, const uint8_t* actions, const float* reward,
                    const uint8_t* boards_s2, const uint8_t* done, int64_t B, double lr, double gamma, uint32_t* status,
                    void*) {
  if (int e = check_lt_update(weights, boards_s, actions, reward, boards_s2, done, B, lr, gamma, status)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      const int act = actions[i];
      if (act > 3) { status_or(status, Q2048_STATUS_BAD_ACTION); continue; }
      Board b_s, b_n;
      load_board(boards_s, i, b_s);
      load_board(boards_s2, i, b_n);
      const Row qn = lt_q(lt_gather(weights, lt_indices(b_n)));
      const LtIdx xs = lt_indices(b_s);
      const LtRows es = lt_gather(weights, xs);
      const float d = lt_delta(row_get(lt_q(es), act), reward[i], max4(qn.q0, qn.q1, qn.q2, qn.q3), done[i] != 0, lr, gamma);
      lt_scatter(weights, xs, es, act, d);
    }
  });
  return Q2048_OK;
}
int q2048_lt_fused_rollout(uint8_t* boards, q2048_aux* aux, float* weights, int64_t B, int64_t steps, double eps,
                           double lr, double gamma, uint64_t seed, uint64_t env_id0, uint32_t ctr0, int64_t* stats_i,
                           double* stats_f, uint32_t* status, void*) {
  if (int e = check_lt_fused(boards, aux, weights, B, steps, eps, lr, gamma, status)) return e;
  if (B == 0 || steps == 0) return Q2048_OK;
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
    Stats& st = sp[tid];
    for (int64_t i = lo; i < hi; ++i) {
      const uint64_t id = env_id0 + (uint64_t)i;
      Board b;
      load_board(boards, i, b);
      Aux a = ld_aux(aux, i);
      double reward_sum = 0.0;
      LtIdx xs = lt_indices(b);
      LtRows es = lt_gather(weights, xs);
      for (int64_t t = 0; t < steps; ++t) {
        const Draws x = draws(seed, id, ctr0 + (uint32_t)t, kStreamStep);
        const Row q = lt_q(es);
        bool explored;
        const int act = eps_greedy(eps, x.x0, x.x1, q.q0, q.q1, q.q2, q.q3, explored);
        const StepOut o = env_step(b, a, act, x.x2, x.x3);
        const LtIdx xn = lt_indices(b);
        LtRows en = lt_gather(weights, xn);
        const Row qn = lt_q(en);
        const float d = lt_delta(row_get(q, act), o.reward, max4(qn.q0, qn.q1, qn.q2, qn.q3), o.done != 0, lr, gamma);
        lt_scatter(weights, xs, es, act, d);
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        reward_sum += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          begin_episode(b, a, seed, id);
          xs = lt_indices(b);
          es = lt_gather(weights, xs);
        } else {
          for (int f = 0; f < kLtFeatures; ++f)
            if (xn.i[f] == xs.i[f]) row_set(en.e[f], act, row_get(es.e[f], act) + d);
          es = en;
          xs = xn;
        }
      }
      st.i[Q2048_ST_STEPS] += (uint64_t)steps;
      st.f[Q2048_SF_REWARD] += reward_sum;
      store_board(boards, i, b);
      st_aux(aux, i, a);
    }
  });
  stats_merge(parts, used, stats_i, stats_f);
  return Q2048_OK;
}
int q2048_lt_play_rollout(uint8_t* boards, q2048_aux* aux, const float* weights, int64_t B, int64_t steps, double eps,
                          uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t* stats_i,
                          double* stats_f, uint32_t* status, void*) {
  if (int e = check_rt_play(boards, aux, weights, B, steps, eps, flags, status)) return e;
  return play_loop(boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f, LtEvalOf{weights});
}

// ---- the afterstate value family: one evaluation = the four moved boards and their 32 entries ----
int q2048_av_value(const float* weights, const uint8_t* boards, int64_t B, float* v_out, void*) {
  if (int e = check_av_value(weights, boards, B, v_out)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      AvTaken t;
      t.x = lt_indices(b);
      av_gather8(weights, t);
      v_out[i] = av_v(t.e);
    }
  });
  return Q2048_OK;
}
int q2048_av_lookup(const float* weights, const uint8_t* boards, int64_t B, float* q_out, void*) {
  if (int e = check_av_lookup(weights, boards, B, q_out)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const Row q = av_row(av_eval(weights, b));
      q_out[4 * i] = q.q0; q_out[4 * i + 1] = q.q1; q_out[4 * i + 2] = q.q2; q_out[4 * i + 3] = q.q3;
    }
  });
  return Q2048_OK;
}
int q2048_av_choose(const float* weights, const uint8_t* boards, int64_t B, double eps, uint64_t seed, uint64_t env_id0,
                    uint32_t ctr, uint8_t* actions, void*) {
  if (int e = check_av_choose(weights, boards, B, eps, actions)) return e;
  const uint64_t eps_t = eps_threshold(eps);
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const Draws x = draws(seed, env_id0 + (uint64_t)i, ctr, kStreamStep);
      const AvEval ev = av_eval(weights, b);
      const Row q = av_row(ev);
      bool explored;
      actions[i] = (uint8_t)play_action(ev.c.legal, q.q0, q.q1, q.q2, q.q3, eps_t, x.x0, x.x1, explored);
    }
  });
  return Q2048_OK;
}
int q2048_av_update(float* weights, const uint8_t* boards_s, const uint8_t* actions, const uint8_t* boards_s2,
                    const uint8_t* done, int64_t B, double lr, double gamma, uint32_t* status, void*) {
  if (int e = check_av_update(weights, boards_s, actions, boards_s2, done, B, lr, gamma, status)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      const int act = actions[i];
      if (act > 3) { status_or(status, Q2048_STATUS_BAD_ACTION); continue; }
      Board b_s, b_st, b_n;
      load_board(boards_s, i, b_s);
      load_board(boards_s2, i, b_n);
      uint32_t score;
      if (!move_with_transpose(b_s, b_st, act, score)) continue;   // the step on which the env reports the end
      const AvEval en = av_eval(weights, b_n);
      AvTaken t;
      t.x = lt_indices_of(b_s, b_st);
      av_gather8(weights, t);
      const bool live = done[i] == 0 && en.c.legal != 0u;
      av_scatter(weights, t, av_delta(av_v(t.e), av_best(en.c.legal, av_row(en)), live, lr, gamma));
    }
  });
  return Q2048_OK;
}
int q2048_av_fused_rollout(uint8_t* boards, q2048_aux* aux, float* weights, int64_t B, int64_t steps, double eps,
                           double lr, double gamma, uint64_t seed, uint64_t env_id0, uint32_t ctr0, int64_t* stats_i,
                           double* stats_f, uint32_t* status, void*) {
  if (int e = check_av_fused(boards, aux, weights, B, steps, eps, lr, gamma, status)) return e;
  if (B == 0 || steps == 0) return Q2048_OK;
  const uint64_t eps_t = eps_threshold(eps);
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
    Stats& st = sp[tid];
    for (int64_t i = lo; i < hi; ++i) {
      const uint64_t id = env_id0 + (uint64_t)i;
      Board b;
      load_board(boards, i, b);
      Aux a = ld_aux(aux, i);
      double reward_sum = 0.0;
      AvEval ev = av_eval(weights, b);
      for (int64_t t = 0; t < steps; ++t) {
        const Draws x = draws(seed, id, ctr0 + (uint32_t)t, kStreamStep);
        const Row q = av_row(ev);
        bool explored;
        const int act = play_action(ev.c.legal, q.q0, q.q1, q.q2, q.q3, eps_t, x.x0, x.x1, explored);
        const bool legal = ((ev.c.legal >> act) & 1u) != 0u;
        const AvTaken tk = av_taken(ev, act);
        const StepOut o = env_step(b, a, act, x.x2, x.x3);
        AvEval en = av_eval(weights, b);
        float d = 0.0f;
        if (legal) {
          const bool live = o.done == 0 && en.c.legal != 0u;
          d = av_delta(av_v(tk.e), av_best(en.c.legal, av_row(en)), live, lr, gamma);
          av_scatter(weights, tk, d);
        }
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        reward_sum += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          begin_episode(b, a, seed, id);
          ev = av_eval(weights, b);
        } else {
          if (legal) av_carry(en, tk, d);
          ev = en;
        }
      }
      st.i[Q2048_ST_STEPS] += (uint64_t)steps;
      st.f[Q2048_SF_REWARD] += reward_sum;
      store_board(boards, i, b);
      st_aux(aux, i, a);
    }
  });
  stats_merge(parts, used, stats_i, stats_f);
  return Q2048_OK;
}
int q2048_av_play_rollout(uint8_t* boards, q2048_aux* aux, const float* weights, int64_t B, int64_t steps, double eps,
                          uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t* stats_i,
                          double* stats_f, uint32_t* status, void*) {
  if (int e = check_av_play(boards, aux, weights, B, steps, eps, flags, status)) return e;
  return play_loop(boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f, AvEvalOf{weights});
}

// ---- the 6-tuple afterstate network: one evaluation = the four moved boards and their 4 x 32 entries; nothing is
// carried from step to step, the fused learner evaluates s from memory on every step ----
int q2048_nt_value(const float* weights, const uint8_t* boards, int64_t B, float* v_out, void*) {
  if (int e = check_nt_value(weights, boards, B, v_out)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      v_out[i] = nt_v(nt_gather(nt_indices(b), NtLd{weights}));
    }
  });
  return Q2048_OK;
}
int q2048_nt_lookup(const float* weights, const uint8_t* boards, int64_t B, float* q_out, void*) {
  if (int e = check_nt_lookup(weights, boards, B, q_out)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const Row q = nt_eval(b, NtLd{weights}).q;
      q_out[4 * i] = q.q0; q_out[4 * i + 1] = q.q1; q_out[4 * i + 2] = q.q2; q_out[4 * i + 3] = q.q3;
    }
  });
  return Q2048_OK;
}
int q2048_nt_choose(const float* weights, const uint8_t* boards, int64_t B, double eps, uint64_t seed, uint64_t env_id0,
                    uint32_t ctr, uint8_t* actions, void*) {
  if (int e = check_nt_choose(weights, boards, B, eps, actions)) return e;
  const uint64_t eps_t = eps_threshold(eps);
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const Draws x = draws(seed, env_id0 + (uint64_t)i, ctr, kStreamStep);
      const NtEval ev = nt_eval(b, NtLd{weights});
      bool explored;
      actions[i] = (uint8_t)play_action(ev.legal, ev.q.q0, ev.q.q1, ev.q.q2, ev.q.q3, eps_t, x.x0, x.x1, explored);
    }
  });
  return Q2048_OK;
}
int q2048_nt_update(float* weights, const uint8_t* boards_s, const uint8_t* actions, const uint8_t* boards_s2,
                    const uint8_t* done, int64_t B, double lr, double gamma, uint32_t* status, void*) {
  if (int e = check_nt_update(weights, boards_s, actions, boards_s2, done, B, lr, gamma, status)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      const int act = actions[i];
      if (act > 3) { status_or(status, Q2048_STATUS_BAD_ACTION); continue; }
      Board x, b_n;
      load_board(boards_s, i, x);
      load_board(boards_s2, i, b_n);
      uint32_t score;
      if (!move(x, act, score)) continue;   // the step on which the env reports the end
      const NtEval en = nt_eval(b_n, NtLd{weights});
      nt_td(x, en, done[i] != 0, lr, gamma, NtLd{weights}, NtSt{weights});
    }
  });
  return Q2048_OK;
}
int q2048_nt_fused_rollout(uint8_t* boards, q2048_aux* aux, float* weights, int64_t B, int64_t steps, double eps,
                           double lr, double gamma, uint64_t seed, uint64_t env_id0, uint32_t ctr0, int64_t* stats_i,
                           double* stats_f, uint32_t* status, void*) {
  if (int e = check_nt_fused(boards, aux, weights, B, steps, eps, lr, gamma, status)) return e;
  if (B == 0 || steps == 0) return Q2048_OK;
  const uint64_t eps_t = eps_threshold(eps);
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
    Stats& st = sp[tid];
    for (int64_t i = lo; i < hi; ++i) {
      const uint64_t id = env_id0 + (uint64_t)i;
      Board b;
      load_board(boards, i, b);
      Aux a = ld_aux(aux, i);
      double reward_sum = 0.0;
      for (int64_t t = 0; t < steps; ++t) {
        const Draws x = draws(seed, id, ctr0 + (uint32_t)t, kStreamStep);
        const NtEval ev = nt_eval(b, NtLd{weights});
        bool explored;
        const int act = play_action(ev.legal, ev.q.q0, ev.q.q1, ev.q.q2, ev.q.q3, eps_t, x.x0, x.x1, explored);
        Board c = b;                    // the afterstate of the move played
        uint32_t score;
        const bool legal = move(c, act, score);
        const StepOut o = env_step(b, a, act, x.x2, x.x3);
        const NtEval en = nt_eval(b, NtLd{weights});
        if (legal) nt_td(c, en, o.done != 0, lr, gamma, NtLd{weights}, NtSt{weights});
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        reward_sum += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          begin_episode(b, a, seed, id);
        }
      }
      st.i[Q2048_ST_STEPS] += (uint64_t)steps;
      st.f[Q2048_SF_REWARD] += reward_sum;
      store_board(boards, i, b);
      st_aux(aux, i, a);
    }
  });
  stats_merge(parts, used, stats_i, stats_f);
  return Q2048_OK;
}
// ---- TD(lambda): q2048_nt_update / q2048_nt_fused_rollout with nt_lambda_td for nt_td and the lane's trace ----
int q2048_nt_choose_ex(const float* weights, const uint8_t* boards, int64_t B, double eps, uint64_t seed, uint64_t env_id0,
                       uint32_t ctr, uint8_t* actions, uint8_t* explored_out, void*) {
  if (int e = check_nt_choose(weights, boards, B, eps, actions)) return e;
  const uint64_t eps_t = eps_threshold(eps);
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const Draws x = draws(seed, env_id0 + (uint64_t)i, ctr, kStreamStep);
      const NtEval ev = nt_eval(b, NtLd{weights});
      bool explored;
      actions[i] = (uint8_t)play_action(ev.legal, ev.q.q0, ev.q.q1, ev.q.q2, ev.q.q3, eps_t, x.x0, x.x1, explored);
      if (explored_out != nullptr) explored_out[i] = explored ? 1 : 0;
    }
  });
  return Q2048_OK;
}
static inline NtTrace ld_trace(const uint64_t* trace, int64_t i) {
  return nt_trace_from(trace[4 * i], trace[4 * i + 1], trace[4 * i + 2], trace[4 * i + 3]);
}
static inline void st_trace(uint64_t* trace, int64_t i, const NtTrace& tr) { nt_trace_words(tr, trace + 4 * i); }
int q2048_nt_lambda_update(float* weights, uint64_t* trace, const uint8_t* boards_s, const uint8_t* actions,
                           const uint8_t* boards_s2, const uint8_t* done, const uint8_t* cut, int64_t B, double lr,
                           double gamma, double lambda, int h, uint32_t* status, void* stream) {
  if (int e = check_nt_lambda_update(weights, trace, boards_s, actions, boards_s2, done, B, lr, gamma, lambda, h, status))
    return e;
  if (h == 0) return q2048_nt_update(weights, boards_s, actions, boards_s2, done, B, lr, gamma, status, stream);
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      const int act = actions[i];
      if (act > 3) { status_or(status, Q2048_STATUS_BAD_ACTION); continue; }
      Board x, b_n;
      load_board(boards_s, i, x);
      load_board(boards_s2, i, b_n);
      const bool over = done[i] != 0;
      NtTrace tr = ld_trace(trace, i);
      uint32_t score;
      if (!move(x, act, score)) {         // the step on which the env reports the end: no weight moves, the trace ends
        if (over) { nt_trace_clear(tr); st_trace(trace, i, tr); }
        continue;
      }
      const NtEval en = nt_eval(b_n, NtLd{weights});
      nt_lambda_td(x, en, over, cut != nullptr && cut[i] != 0, lr, gamma, lambda, (uint32_t)h, tr, NtLd{weights},
                   NtSt{weights});
      st_trace(trace, i, tr);
    }
  });
  return Q2048_OK;
}
int q2048_nt_lambda_fused_rollout(uint8_t* boards, q2048_aux* aux, float* weights, uint64_t* trace, int64_t B,
                                  int64_t steps, double eps, double lr, double gamma, double lambda, int h,
                                  uint64_t seed, uint64_t env_id0, uint32_t ctr0, int64_t* stats_i, double* stats_f,
                                  uint32_t* status, void* stream) {
  if (int e = check_nt_lambda_fused(boards, aux, weights, trace, B, steps, eps, lr, gamma, lambda, h, status)) return e;
  if (B == 0 || steps == 0) return Q2048_OK;
  if (h == 0)
    return q2048_nt_fused_rollout(boards, aux, weights, B, steps, eps, lr, gamma, seed, env_id0, ctr0, stats_i, stats_f,
                                  status, stream);
  const uint64_t eps_t = eps_threshold(eps);
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
    Stats& st = sp[tid];
    for (int64_t i = lo; i < hi; ++i) {
      const uint64_t id = env_id0 + (uint64_t)i;
      Board b;
      load_board(boards, i, b);
      Aux a = ld_aux(aux, i);
      NtTrace tr = ld_trace(trace, i);
      double reward_sum = 0.0;
      for (int64_t t = 0; t < steps; ++t) {
        const Draws x = draws(seed, id, ctr0 + (uint32_t)t, kStreamStep);
        const NtEval ev = nt_eval(b, NtLd{weights});
        bool explored;
        const int act = play_action(ev.legal, ev.q.q0, ev.q.q1, ev.q.q2, ev.q.q3, eps_t, x.x0, x.x1, explored);
        Board c = b;                    // the afterstate of the move played
        uint32_t score;
        const bool legal = move(c, act, score);
        const StepOut o = env_step(b, a, act, x.x2, x.x3);
        const NtEval en = nt_eval(b, NtLd{weights});
        if (legal) nt_lambda_td(c, en, o.done != 0, explored, lr, gamma, lambda, (uint32_t)h, tr, NtLd{weights}, NtSt{weights});
        else if (o.done) nt_trace_clear(tr);
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        reward_sum += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          begin_episode(b, a, seed, id);
        }
      }
      st.i[Q2048_ST_STEPS] += (uint64_t)steps;
      st.f[Q2048_SF_REWARD] += reward_sum;
      store_board(boards, i, b);
      st_aux(aux, i, a);
      st_trace(trace, i, tr);
    }
  });
  stats_merge(parts, used, stats_i, stats_f);
  return Q2048_OK;
}
// ---- the synchronous batch step: phase A over the thread ranges, a join, phase B over the same ranges ----
int q2048_nt_sync_update(float* weights, uint64_t* acc, const uint8_t* boards_s, const uint8_t* actions,
                         const uint8_t* boards_s2, const uint8_t* done, int64_t B, double lr, double gamma,
                         uint32_t* status, void*) {
  if (int e = check_nt_sync_update(weights, acc, boards_s, actions, boards_s2, done, B, lr, gamma, status)) return e;
  if (B == 0) return Q2048_OK;
  std::vector<uint64_t> keys((size_t)B);      // the afterstate each lane contributed, 0 = none
  uint64_t* kp = keys.data();
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      kp[i] = 0ull;
      const int act = actions[i];
      if (act > 3) { status_or(status, Q2048_STATUS_BAD_ACTION); continue; }
      Board x, b_n;
      load_board(boards_s, i, x);
      load_board(boards_s2, i, b_n);
      uint32_t score;
      if (!move(x, act, score)) continue;   // the step on which the env reports the end
      const NtEval en = nt_eval(b_n, NtLd{weights});
      kp[i] = nt_sync_acc(x, en, done[i] != 0, gamma, NtLd{weights}, NtSyncAdd{acc});
    }
  });
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i)
      if (kp[i] != 0ull) nt_sync_apply(kp[i], lr, NtLd{weights}, NtSt{weights}, NtSyncClaim{acc}, NtSyncTake{acc});
  });
  return Q2048_OK;
}
int q2048_nt_sync_fused_rollout(uint8_t* boards, q2048_aux* aux, float* weights, uint64_t* acc, uint64_t* pend, int64_t B,
                                int64_t steps, double eps, double lr, double gamma, uint64_t seed, uint64_t env_id0,
                                uint32_t ctr0, int64_t* stats_i, double* stats_f, uint32_t* status, void*) {
  if (int e = check_nt_sync_fused(boards, aux, weights, acc, pend, B, steps, eps, lr, gamma, status)) return e;
  if (B == 0 || steps == 0) return Q2048_OK;
  const uint64_t eps_t = eps_threshold(eps);
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  int used = 0;
  for (int64_t t = 0; t < steps; ++t) {
    used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
      Stats& st = sp[tid];
      for (int64_t i = lo; i < hi; ++i) {
        const uint64_t id = env_id0 + (uint64_t)i;
        Board b;
        load_board(boards, i, b);
        Aux a = ld_aux(aux, i);
        const Draws x = draws(seed, id, ctr0 + (uint32_t)t, kStreamStep);
        const NtEval ev = nt_eval(b, NtLd{weights});
        bool explored;
        const int act = play_action(ev.legal, ev.q.q0, ev.q.q1, ev.q.q2, ev.q.q3, eps_t, x.x0, x.x1, explored);
        Board c = b;                    // the afterstate of the move played
        uint32_t score;
        const bool legal = move(c, act, score);
        const StepOut o = env_step(b, a, act, x.x2, x.x3);
        const NtEval en = nt_eval(b, NtLd{weights});
        pend[i] = legal ? nt_sync_acc(c, en, o.done != 0, gamma, NtLd{weights}, NtSyncAdd{acc}) : 0ull;
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        st.i[Q2048_ST_STEPS] += 1;
        st.f[Q2048_SF_REWARD] += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          begin_episode(b, a, seed, id);
        }
        store_board(boards, i, b);
        st_aux(aux, i, a);
      }
    });
    parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
      for (int64_t i = lo; i < hi; ++i) {
        const uint64_t key = pend[i];
        pend[i] = 0ull;
        if (key != 0ull) nt_sync_apply(key, lr, NtLd{weights}, NtSt{weights}, NtSyncClaim{acc}, NtSyncTake{acc});
      }
    });
  }
  stats_merge(parts, used, stats_i, stats_f);
  return Q2048_OK;
}
// ---- temporal-coherence step sizes: q2048_nt_update / q2048_nt_fused_rollout with nt_tc_td for nt_td ----
int q2048_nt_tc_update(float* weights, float* acc, const uint8_t* boards_s, const uint8_t* actions,
                       const uint8_t* boards_s2, const uint8_t* done, int64_t B, double lr, double gamma,
                       uint32_t* status, void*) {
  if (int e = check_nt_tc_update(weights, acc, boards_s, actions, boards_s2, done, B, lr, gamma, status)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      const int act = actions[i];
      if (act > 3) { status_or(status, Q2048_STATUS_BAD_ACTION); continue; }
      Board x, b_n;
      load_board(boards_s, i, x);
      load_board(boards_s2, i, b_n);
      uint32_t score;
      if (!move(x, act, score)) continue;   // the step on which the env reports the end
      const NtEval en = nt_eval(b_n, NtLd{weights});
      nt_tc_td(x, en, done[i] != 0, lr, gamma, NtLd{weights}, NtTcLd{acc}, NtSt{weights}, NtTcSt{acc});
    }
  });
  return Q2048_OK;
}
int q2048_nt_tc_fused_rollout(uint8_t* boards, q2048_aux* aux, float* weights, float* acc, int64_t B, int64_t steps,
                              double eps, double lr, double gamma, uint64_t seed, uint64_t env_id0, uint32_t ctr0,
                              int64_t* stats_i, double* stats_f, uint32_t* status, void*) {
  if (int e = check_nt_tc_fused(boards, aux, weights, acc, B, steps, eps, lr, gamma, status)) return e;
  if (B == 0 || steps == 0) return Q2048_OK;
  const uint64_t eps_t = eps_threshold(eps);
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
    Stats& st = sp[tid];
    for (int64_t i = lo; i < hi; ++i) {
      const uint64_t id = env_id0 + (uint64_t)i;
      Board b;
      load_board(boards, i, b);
      Aux a = ld_aux(aux, i);
      double reward_sum = 0.0;
      for (int64_t t = 0; t < steps; ++t) {
        const Draws x = draws(seed, id, ctr0 + (uint32_t)t, kStreamStep);
        const NtEval ev = nt_eval(b, NtLd{weights});
        bool explored;
        const int act = play_action(ev.legal, ev.q.q0, ev.q.q1, ev.q.q2, ev.q.q3, eps_t, x.x0, x.x1, explored);
        Board c = b;                    // the afterstate of the move played
        uint32_t score;
        const bool legal = move(c, act, score);
        const StepOut o = env_step(b, a, act, x.x2, x.x3);
        const NtEval en = nt_eval(b, NtLd{weights});
        if (legal) nt_tc_td(c, en, o.done != 0, lr, gamma, NtLd{weights}, NtTcLd{acc}, NtSt{weights}, NtTcSt{acc});
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        reward_sum += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          begin_episode(b, a, seed, id);
        }
      }
      st.i[Q2048_ST_STEPS] += (uint64_t)steps;
      st.f[Q2048_SF_REWARD] += reward_sum;
      store_board(boards, i, b);
      st_aux(aux, i, a);
    }
  });
  stats_merge(parts, used, stats_i, stats_f);
  return Q2048_OK;
}
int q2048_nt_play_rollout(uint8_t* boards, q2048_aux* aux, const float* weights, int64_t B, int64_t steps, double eps,
                          uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t* stats_i,
                          double* stats_f, uint32_t* status, void*) {
  if (int e = check_nt_play(boards, aux, weights, B, steps, eps, flags, status)) return e;
  return play_loop(boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f, NtEvalOf{weights});
}

// ---- one-level expectimax over the spawn: the players above with the searched row (search_row, q2048_core.hpp) ----
int q2048_av_search_lookup(const float* weights, const uint8_t* boards, int64_t B, float* q_out, uint8_t* legal_out, void*) {
  if (int e = check_search_lookup(weights, boards, B, q_out, legal_out)) return e;
  return search_lookup_impl<1>(AvEvalOf{weights}, boards, B, q_out, legal_out);
}
int q2048_av_search_play_rollout(uint8_t* boards, q2048_aux* aux, const float* weights, int64_t B, int64_t steps, double eps,
                                 uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t* stats_i,
                                 double* stats_f, uint32_t* status, void*) {
  if (int e = check_search_play(boards, aux, weights, B, steps, eps, flags, status)) return e;
  return search_play_impl(AvEvalOf{weights}, 1, boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f);
}
int q2048_nt_search_lookup(const float* weights, const uint8_t* boards, int64_t B, float* q_out, uint8_t* legal_out, void*) {
  if (int e = check_search_lookup(weights, boards, B, q_out, legal_out)) return e;
  return search_lookup_impl<1>(NtEvalOf{weights}, boards, B, q_out, legal_out);
}
int q2048_nt_search_play_rollout(uint8_t* boards, q2048_aux* aux, const float* weights, int64_t B, int64_t steps, double eps,
                                 uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t* stats_i,
                                 double* stats_f, uint32_t* status, void*) {
  if (int e = check_search_play(boards, aux, weights, B, steps, eps, flags, status)) return e;
  return search_play_impl(NtEvalOf{weights}, 1, boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f);
}
// ---- the same with a search depth: 1 = the functions above, 2 = the two-level row (search_row2, q2048_core.hpp) ----
int q2048_av_search_lookup_depth(const float* weights, const uint8_t* boards, int64_t B, int depth, float* q_out,
                                 uint8_t* legal_out, void*) {
  if (int e = check_search_lookup_depth(weights, boards, B, depth, q_out, legal_out)) return e;
  return search_lookup_depth(AvEvalOf{weights}, depth, boards, B, q_out, legal_out);
}
int q2048_av_search_play_rollout_depth(uint8_t* boards, q2048_aux* aux, const float* weights, int64_t B, int64_t steps,
                                       int depth, double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                                       int64_t* stats_i, double* stats_f, uint32_t* status, void*) {
  if (int e = check_search_play_depth(boards, aux, weights, B, steps, depth, eps, flags, status)) return e;
  return search_play_impl(AvEvalOf{weights}, depth, boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f);
}
int q2048_nt_search_lookup_depth(const float* weights, const uint8_t* boards, int64_t B, int depth, float* q_out,
                                 uint8_t* legal_out, void*) {
  if (int e = check_search_lookup_depth(weights, boards, B, depth, q_out, legal_out)) return e;
  return search_lookup_depth(NtEvalOf{weights}, depth, boards, B, q_out, legal_out);
}
int q2048_nt_search_play_rollout_depth(uint8_t* boards, q2048_aux* aux, const float* weights, int64_t B, int64_t steps,
                                       int depth, double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                                       int64_t* stats_i, double* stats_f, uint32_t* status, void*) {
  if (int e = check_search_play_depth(boards, aux, weights, B, steps, depth, eps, flags, status)) return e;
  return search_play_impl(NtEvalOf{weights}, depth, boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f);
}

// ---- the staged network (q2048_nts_*): the functions above with nts_eval / nts_td, the table picked per candidate ----
int q2048_nts_value(const float* weights, uint32_t stages, const uint8_t* boards, int64_t B, float* v_out, void*) {
  if (int e = check_nts_value(weights, stages, boards, B, v_out)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      v_out[i] = nts_v(b, stages, NtsLdOf{weights});
    }
  });
  return Q2048_OK;
}
int q2048_nts_lookup(const float* weights, uint32_t stages, const uint8_t* boards, int64_t B, float* q_out, void*) {
  if (int e = check_nts_lookup(weights, stages, boards, B, q_out)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const Row q = nts_eval(b, stages, NtsLdOf{weights}).q;
      q_out[4 * i] = q.q0; q_out[4 * i + 1] = q.q1; q_out[4 * i + 2] = q.q2; q_out[4 * i + 3] = q.q3;
    }
  });
  return Q2048_OK;
}
int q2048_nts_choose(const float* weights, uint32_t stages, const uint8_t* boards, int64_t B, double eps, uint64_t seed,
                     uint64_t env_id0, uint32_t ctr, uint8_t* actions, void*) {
  if (int e = check_nts_choose(weights, stages, boards, B, eps, actions)) return e;
  const uint64_t eps_t = eps_threshold(eps);
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      Board b;
      load_board(boards, i, b);
      const Draws x = draws(seed, env_id0 + (uint64_t)i, ctr, kStreamStep);
      const NtEval ev = nts_eval(b, stages, NtsLdOf{weights});
      bool explored;
      actions[i] = (uint8_t)play_action(ev.legal, ev.q.q0, ev.q.q1, ev.q.q2, ev.q.q3, eps_t, x.x0, x.x1, explored);
    }
  });
  return Q2048_OK;
}
int q2048_nts_update(float* weights, uint32_t stages, const uint8_t* boards_s, const uint8_t* actions,
                     const uint8_t* boards_s2, const uint8_t* done, int64_t B, double lr, double gamma, uint32_t* status,
                     void*) {
  if (int e = check_nts_update(weights, stages, boards_s, actions, boards_s2, done, B, lr, gamma, status)) return e;
  parallel_ranges(B, [=](int64_t lo, int64_t hi, int) {
    for (int64_t i = lo; i < hi; ++i) {
      const int act = actions[i];
      if (act > 3) { status_or(status, Q2048_STATUS_BAD_ACTION); continue; }
      Board x, b_n;
      load_board(boards_s, i, x);
      load_board(boards_s2, i, b_n);
      uint32_t score;
      if (!move(x, act, score)) continue;   // the step on which the env reports the end
      const NtEval en = nts_eval(b_n, stages, NtsLdOf{weights});
      nts_td(x, stages, en, done[i] != 0, lr, gamma, NtsLdOf{weights}, NtsStOf{weights});
    }
  });
  return Q2048_OK;
}
int q2048_nts_fused_rollout(uint8_t* boards, q2048_aux* aux, float* weights, uint32_t stages, int64_t B, int64_t steps,
                            double eps, double lr, double gamma, uint64_t seed, uint64_t env_id0, uint32_t ctr0,
                            int64_t* stats_i, double* stats_f, uint32_t* status, void*) {
  if (int e = check_nts_fused(boards, aux, weights, stages, B, steps, eps, lr, gamma, status)) return e;
  if (B == 0 || steps == 0) return Q2048_OK;
  const uint64_t eps_t = eps_threshold(eps);
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
    Stats& st = sp[tid];
    for (int64_t i = lo; i < hi; ++i) {
      const uint64_t id = env_id0 + (uint64_t)i;
      Board b;
      load_board(boards, i, b);
      Aux a = ld_aux(aux, i);
      double reward_sum = 0.0;
      for (int64_t t = 0; t < steps; ++t) {
        const Draws x = draws(seed, id, ctr0 + (uint32_t)t, kStreamStep);
        const NtEval ev = nts_eval(b, stages, NtsLdOf{weights});
        bool explored;
        const int act = play_action(ev.legal, ev.q.q0, ev.q.q1, ev.q.q2, ev.q.q3, eps_t, x.x0, x.x1, explored);
        Board c = b;                    // the afterstate of the move played
        uint32_t score;
        const bool legal = move(c, act, score);
        const StepOut o = env_step(b, a, act, x.x2, x.x3);
        const NtEval en = nts_eval(b, stages, NtsLdOf{weights});
        if (legal) nts_td(c, stages, en, o.done != 0, lr, gamma, NtsLdOf{weights}, NtsStOf{weights});
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        reward_sum += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          begin_episode(b, a, seed, id);
        }
      }
      st.i[Q2048_ST_STEPS] += (uint64_t)steps;
      st.f[Q2048_SF_REWARD] += reward_sum;
      store_board(boards, i, b);
      st_aux(aux, i, a);
    }
  });
  stats_merge(parts, used, stats_i, stats_f);
  return Q2048_OK;
}
// ---- carousel shaping (q2048_car_*; the contract is "CAROUSEL SHAPING" in q2048_core.hpp) ----
// q2048_nts_fused_rollout with the recording test after env_step and car_restart for begin_episode
int q2048_car_fused_rollout(uint8_t* boards, q2048_aux* aux, float* weights, uint32_t stages, const uint8_t* pool,
                            const uint64_t* counts, uint8_t* fresh, int64_t P, int64_t B, int64_t steps, double eps,
                            double lr, double gamma, uint64_t seed, uint64_t env_id0, uint32_t ctr0, int64_t* stats_i,
                            double* stats_f, uint32_t* status, void*) {
  if (int e = check_car_fused(boards, aux, weights, stages, pool, counts, fresh, P, B, steps, eps, lr, gamma, status))
    return e;
  if (B == 0 || steps == 0) return Q2048_OK;
  const uint64_t eps_t = eps_threshold(eps);
  const uint32_t S = nts_count(stages);
  const int T = threads_for(B);
  std::vector<Stats> parts((size_t)T);
  Stats* sp = parts.data();
  const int used = parallel_ranges(B, [=](int64_t lo, int64_t hi, int tid) {
    Stats& st = sp[tid];
    const auto valid = [=](uint32_t k) { return car_valid(counts[k], (uint64_t)P); };
    const auto ld_rec = [=](uint32_t k, uint32_t j) {
      CarRecord rec;
      std::memcpy(&rec, pool + ((size_t)k * (size_t)P + j) * kCarRecordBytes, kCarRecordBytes);
      return rec;
    };
    for (int64_t i = lo; i < hi; ++i) {
      const uint64_t id = env_id0 + (uint64_t)i;
      Board b;
      load_board(boards, i, b);
      Aux a = ld_aux(aux, i);
      double reward_sum = 0.0;
      for (int64_t t = 0; t < steps; ++t) {
        const Draws x = draws(seed, id, ctr0 + (uint32_t)t, kStreamStep);
        const NtEval ev = nts_eval(b, stages, NtsLdOf{weights});
        bool explored;
        const int act = play_action(ev.legal, ev.q.q0, ev.q.q1, ev.q.q2, ev.q.q3, eps_t, x.x0, x.x1, explored);
        Board c = b;                    // the afterstate of the move played
        uint32_t score;
        const bool legal = move(c, act, score);
        const uint32_t k0 = nts_stage(b, stages);
        const StepOut o = env_step(b, a, act, x.x2, x.x3);
        const uint32_t k1 = nts_stage(b, stages);
        if (car_records(k0, k1, o.done != 0)) {
          const CarRecord rec = car_record(b, a);
          std::memcpy(fresh + ((size_t)k1 * (size_t)B + (size_t)i) * kCarRecordBytes, &rec, kCarRecordBytes);
        }
        const NtEval en = nts_eval(b, stages, NtsLdOf{weights});
        if (legal) nts_td(c, stages, en, o.done != 0, lr, gamma, NtsLdOf{weights}, NtsStOf{weights});
        st.i[Q2048_ST_VALID] += o.valid != 0;
        st.i[Q2048_ST_EXPLORE] += explored;
        reward_sum += (double)o.reward;
        if (o.done) {
          st.i[Q2048_ST_EPISODES] += 1;
          st.episode(a, o.max_log2);
          car_restart(b, a, seed, id, S, valid, ld_rec);
        }
      }
      st.i[Q2048_ST_STEPS] += (uint64_t)steps;
      st.f[Q2048_SF_REWARD] += reward_sum;
      store_board(boards, i, b);
      st_aux(aux, i, a);
    }
  });
  stats_merge(parts, used, stats_i, stats_f);
  return Q2048_OK;
}
// the commit, a stage at a time: count the non-empty records, then place them in ascending lane order
int q2048_car_commit(uint8_t* pool, uint64_t* counts, uint8_t* fresh, uint32_t stages, int64_t P, int64_t B, void*) {
  if (int e = check_car_commit(pool, counts, fresh, stages, P, B)) return e;
  if (B == 0) return Q2048_OK;
  const uint32_t S = nts_count(stages);
  static const uint8_t zero[kCarRecordBytes] = {};
  for (uint32_t k = 1; k < S; ++k) {
    uint8_t* rows = fresh + (size_t)k * (size_t)B * kCarRecordBytes;
    const auto empty = [=](int64_t i) {
      Board b;
      std::memcpy(&b, rows + (size_t)i * kCarRecordBytes, sizeof b);
      return car_empty(b);
    };
    uint64_t m = 0;
    for (int64_t i = 0; i < B; ++i) m += !empty(i);
    uint64_t r = 0;
    for (int64_t i = 0; i < B; ++i) {
      if (empty(i)) continue;
      uint8_t* rec = rows + (size_t)i * kCarRecordBytes;
      if (car_lands(r, m, (uint64_t)P))
        std::memcpy(pool + ((size_t)k * (size_t)P + car_slot(counts[k], r, (uint64_t)P)) * kCarRecordBytes, rec,
                    kCarRecordBytes);
      std::memcpy(rec, zero, kCarRecordBytes);
      ++r;
    }
    counts[k] += m;
  }
  return Q2048_OK;
}
int q2048_nts_play_rollout(uint8_t* boards, q2048_aux* aux, const float* weights, uint32_t stages, int64_t B, int64_t steps,
                           double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t* stats_i,
                           double* stats_f, uint32_t* status, void*) {
  if (int e = check_nts_play(boards, aux, weights, stages, B, steps, eps, flags, status)) return e;
  return play_loop(boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i, stats_f, NtsEvalOf{weights, stages});
}
int q2048_nts_search_lookup_depth(const float* weights, uint32_t stages, const uint8_t* boards, int64_t B, int depth,
                                  float* q_out, uint8_t* legal_out, void*) {
  if (int e = check_nts_search_lookup_depth(weights, stages, boards, B, depth, q_out, legal_out)) return e;
  return search_lookup_depth(NtsEvalOf{weights, stages}, depth, boards, B, q_out, legal_out);
}
int q2048_nts_search_play_rollout_depth(uint8_t* boards, q2048_aux* aux, const float* weights, uint32_t stages, int64_t B,
                                        int64_t steps, int depth, double eps, uint64_t seed, uint64_t env_id0,
                                        uint32_t ctr0, uint32_t flags, int64_t* stats_i, double* stats_f,
                                        uint32_t* status, void*) {
  if (int e = check_nts_search_play_depth(boards, aux, weights, stages, B, steps, depth, eps, flags, status)) return e;
  return search_play_impl(NtsEvalOf{weights, stages}, depth, boards, aux, B, steps, eps, seed, env_id0, ctr0, flags, stats_i,
                          stats_f);
}
// promotion: the rule of nts_promotes on every entry, bits in and bits out
int q2048_nts_promote(float* weights, uint32_t stages, int from, int to, int64_t* count_out, void*) {
  if (int e = check_nts_promote(weights, stages, from, to)) return e;
  float* dst = weights + (size_t)to * kNtsStageFloats;
  const float* src = weights + (size_t)from * kNtsStageFloats;
  const int64_t n = (int64_t)kNtsStageFloats;
  std::vector<int64_t> parts((size_t)threads_for(n), 0);
  int64_t* pp = parts.data();
  const int used = parallel_ranges(n, [=](int64_t lo, int64_t hi, int tid) {
    int64_t copied = 0;
    for (int64_t i = lo; i < hi; ++i) {
      uint32_t d, s;
      std::memcpy(&d, dst + i, sizeof d);
      std::memcpy(&s, src + i, sizeof s);
      if (nts_promotes(d, s)) {
        std::memcpy(dst + i, &s, sizeof s);
        ++copied;
      }
    }
    pp[tid] = copied;
  });
  if (count_out != nullptr) {
    int64_t total = 0;
    for (int t = 0; t < used; ++t) total += parts[(size_t)t];
    *count_out = total;
  }
  return Q2048_OK;
}

}  // extern "C"
