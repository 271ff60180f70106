// q2048_abi.hpp -- the argument checks of the C ABI (include/q2048.h) and the text of its error codes.
//
// Host code only, compiled into both libraries (libq2048_hip.so: q2048_kernels.hip; libq2048_host.so:
// q2048_host.cpp), so that an argument one of them refuses the other refuses too, with the same code and in the
// same order of precedence.  Everything has internal linkage: the libraries export the C ABI and nothing of this.
#pragma once
#include <cmath>
#include <cstdint>

#include "q2048.h"
#include "q2048_core.hpp"   // the stage spec of q2048_nts_* (nts_spec_ok, nts_count)

namespace q2048 {

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline int check_batch(int64_t B, int n) {
  if (n != 4 && n != 5) return Q2048_ERR_UNSUPPORTED;
  // the device launches one block per 256 envs and HIP caps grid.x at 2^31 - 1 blocks
  if (B < 0 || B > (int64_t)0x7fffffff * 256) return Q2048_ERR_SIZE;
  return Q2048_OK;
}
static inline int check_table(const void* table, int cap_log2) {
  if (table == nullptr) return Q2048_ERR_NULL;
  if (cap_log2 < 4 || cap_log2 > 40) return Q2048_ERR_SIZE;
  if (!aligned16(table)) return Q2048_ERR_ALIGN;
  return Q2048_OK;
}
// flag bits outside the ABI are an argument error (experiment builds of the HIP library also take bits 8..23).
// (Q2048_FLAG_LINE_SUMMARY on the host: 4x4 accepted and not used -- slot by slot, same results; 5x5 with a side
// array: used.)
constexpr uint32_t kAbiFlags = Q2048_FLAG_INDEPENDENT | Q2048_FLAG_SINGLE_ENV | Q2048_FLAG_TD_CAS |
                               Q2048_FLAG_ENV_DQN | Q2048_FLAG_RESET_SHAPING | Q2048_FLAG_PLAY_ONLY |
                               Q2048_FLAG_NO_LEARN | Q2048_FLAG_NO_NEW_ROWS | Q2048_FLAG_LINE_SUMMARY;
// (`also`: Q2048_FLAG_SYMMETRIC, for the entry points that take it -- the fused rollouts, the player, q_lookup)
static inline int check_flags(uint32_t flags, uint32_t refused = 0u, uint32_t also = 0u) {
  uint32_t allowed = kAbiFlags | also;
#ifdef Q2048_EXPERIMENTS
  allowed |= 0x00ffff00u;
#endif
  return ((flags & ~allowed) || (flags & refused)) ? Q2048_ERR_FLAGS : Q2048_OK;
}

// What q2048_table_merge and q2048_table_fold check in common, in their order of precedence: NULL, SIZE, ALIGN,
// FLAGS, RANGE.  `sizes_ok` / `rules_ok` are the caller's verdict on its own arguments of the same rank as the
// capacities (key_words) / as the merge mode (the fold rule).
static inline int check_merge(const void* dst, int dst_cap_log2, const void* src, int src_cap_log2, const void* counters,
                              bool sizes_ok, bool rules_ok, int mode, float w) {
  if (!dst || !src || !counters) return Q2048_ERR_NULL;
  if (dst_cap_log2 < 4 || dst_cap_log2 > 40 || src_cap_log2 < 4 || src_cap_log2 > 40 || !sizes_ok) return Q2048_ERR_SIZE;
  if (!aligned16(dst) || !aligned16(src)) return Q2048_ERR_ALIGN;
  if (!rules_ok || (mode != Q2048_MERGE_ADD && mode != Q2048_MERGE_BLEND && mode != Q2048_MERGE_MAXABS)) return Q2048_ERR_FLAGS;
  if (!std::isfinite(w) || (mode == Q2048_MERGE_BLEND && !(w >= 0.0f && w <= 1.0f))) return Q2048_ERR_RANGE;
  const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), s0 = reinterpret_cast<uintptr_t>(src);
  const uintptr_t d1 = d0 + (sizeof(q2048_slot) << dst_cap_log2), s1 = s0 + (sizeof(q2048_slot) << src_cap_log2);
  if (s0 < d1 && d0 < s1) return Q2048_ERR_RANGE;                      // the two tables overlap (src == dst included)
  return Q2048_OK;
}

// What q2048_rt_play_rollout checks, in the order of q2048_play_rollout: B, flags (the env-profile bits and nothing
// else: Q2048_FLAG_INDEPENDENT and Q2048_FLAG_SYMMETRIC mean nothing to weights), NULL, alignment, steps, eps.
static inline int check_rt_play(const void* boards, const void* aux, const void* weights, int64_t B, int64_t steps,
                                double eps, uint32_t flags, const void* status) {
  if (int e = check_batch(B, 4)) return e;
  if (int e = check_flags(flags, kAbiFlags & ~(Q2048_FLAG_ENV_DQN | Q2048_FLAG_RESET_SHAPING))) return e;
  if (!boards || !aux || !weights || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux) || !aligned16(weights)) return Q2048_ERR_ALIGN;
  if (steps < 0 || steps > (1 << 30)) return Q2048_ERR_SIZE;
  if (!(eps >= 0.0 && eps <= 1.0)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}

// What the four-call entry points and the fused learner of the line-tuple family check, in the order of their
// q2048_rt_* counterparts: B, NULL, alignment, (steps,) the scalars.
static inline int check_lt_choose(const void* weights, const void* boards, int64_t B, double eps, const void* actions) {
  if (int e = check_batch(B, 4)) return e;
  if (!weights || !boards || !actions) return Q2048_ERR_NULL;
  if (!aligned16(weights) || !aligned16(boards)) return Q2048_ERR_ALIGN;
  if (!(eps >= 0.0 && eps <= 1.0)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}
static inline int check_lt_lookup(const void* weights, const void* boards, int64_t B, const void* q_out) {
  if (int e = check_batch(B, 4)) return e;
  if (!weights || !boards || !q_out) return Q2048_ERR_NULL;
  if (!aligned16(weights) || !aligned16(boards) || !aligned16(q_out)) return Q2048_ERR_ALIGN;
  return Q2048_OK;
}
static inline int check_lt_update(const void* weights, const void* boards_s, const void* actions, const void* reward,
                                  const void* boards_s2, const void* done, int64_t B, double lr, double gamma,
                                  const void* status) {
  if (int e = check_batch(B, 4)) return e;
  if (!weights || !boards_s || !actions || !reward || !boards_s2 || !done || !status) return Q2048_ERR_NULL;
  if (!aligned16(weights) || !aligned16(boards_s) || !aligned16(boards_s2)) return Q2048_ERR_ALIGN;
  if (!(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}
static inline int check_lt_fused(const void* boards, const void* aux, const void* weights, int64_t B, int64_t steps,
                                 double eps, double lr, double gamma, const void* status) {
  if (int e = check_batch(B, 4)) return e;
  if (!boards || !aux || !weights || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux) || !aligned16(weights)) return Q2048_ERR_ALIGN;
  if (steps < 0 || steps > (1 << 30)) return Q2048_ERR_SIZE;
  if (!(eps >= 0.0 && eps <= 1.0) || !(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}

// The afterstate value family (q2048_av_*): order and codes of the lt_ counterparts.  q2048_av_value checks as the
// lookup does; the update has no reward argument; the player checks as q2048_rt_play_rollout does.
static inline int check_av_value(const void* weights, const void* boards, int64_t B, const void* v_out) {
  return check_lt_lookup(weights, boards, B, v_out);
}
static inline int check_av_lookup(const void* weights, const void* boards, int64_t B, const void* q_out) {
  return check_lt_lookup(weights, boards, B, q_out);
}
static inline int check_av_choose(const void* weights, const void* boards, int64_t B, double eps, const void* actions) {
  return check_lt_choose(weights, boards, B, eps, actions);
}
static inline int check_av_update(const void* weights, const void* boards_s, const void* actions, const void* boards_s2,
                                  const void* done, int64_t B, double lr, double gamma, const void* status) {
  if (int e = check_batch(B, 4)) return e;
  if (!weights || !boards_s || !actions || !boards_s2 || !done || !status) return Q2048_ERR_NULL;
  if (!aligned16(weights) || !aligned16(boards_s) || !aligned16(boards_s2)) return Q2048_ERR_ALIGN;
  if (!(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}
static inline int check_av_fused(const void* boards, const void* aux, const void* weights, int64_t B, int64_t steps,
                                 double eps, double lr, double gamma, const void* status) {
  return check_lt_fused(boards, aux, weights, B, steps, eps, lr, gamma, status);
}
static inline int check_av_play(const void* boards, const void* aux, const void* weights, int64_t B, int64_t steps,
                                double eps, uint32_t flags, const void* status) {
  return check_rt_play(boards, aux, weights, B, steps, eps, flags, status);
}

// The 6-tuple afterstate network (q2048_nt_*): the checks of the q2048_av_* counterparts, in their order, with their codes.
static inline int check_nt_value(const void* weights, const void* boards, int64_t B, const void* v_out) {
  return check_av_value(weights, boards, B, v_out);
}
static inline int check_nt_lookup(const void* weights, const void* boards, int64_t B, const void* q_out) {
  return check_av_lookup(weights, boards, B, q_out);
}
static inline int check_nt_choose(const void* weights, const void* boards, int64_t B, double eps, const void* actions) {
  return check_av_choose(weights, boards, B, eps, actions);
}
static inline int check_nt_update(const void* weights, const void* boards_s, const void* actions, const void* boards_s2,
                                  const void* done, int64_t B, double lr, double gamma, const void* status) {
  return check_av_update(weights, boards_s, actions, boards_s2, done, B, lr, gamma, status);
}
static inline int check_nt_fused(const void* boards, const void* aux, const void* weights, int64_t B, int64_t steps,
                                 double eps, double lr, double gamma, const void* status) {
  return check_av_fused(boards, aux, weights, B, steps, eps, lr, gamma, status);
}
static inline int check_nt_play(const void* boards, const void* aux, const void* weights, int64_t B, int64_t steps,
                                double eps, uint32_t flags, const void* status) {
  return check_av_play(boards, aux, weights, B, steps, eps, flags, status);
}

// Temporal-coherence step sizes for the network (q2048_nt_tc_*): the checks of the q2048_nt_* counterparts in their
// order, `acc` directly after `weights` in the NULL and in the alignment list, and after the alignment checks one of
// their own: V (256 MiB) and acc (512 MiB) may not overlap.
static inline bool nt_tc_overlap(const void* weights, const void* acc) {
  const uintptr_t w0 = reinterpret_cast<uintptr_t>(weights), a0 = reinterpret_cast<uintptr_t>(acc);
  const uintptr_t w1 = w0 + ((uintptr_t)1 << 28), a1 = a0 + ((uintptr_t)1 << 29);
  return a0 < w1 && w0 < a1;
}
static inline int check_nt_tc_update(const void* weights, const void* acc, const void* boards_s, const void* actions,
                                     const void* boards_s2, const void* done, int64_t B, double lr, double gamma,
                                     const void* status) {
  if (int e = check_batch(B, 4)) return e;
  if (!weights || !acc || !boards_s || !actions || !boards_s2 || !done || !status) return Q2048_ERR_NULL;
  if (!aligned16(weights) || !aligned16(acc) || !aligned16(boards_s) || !aligned16(boards_s2)) return Q2048_ERR_ALIGN;
  if (nt_tc_overlap(weights, acc)) return Q2048_ERR_RANGE;
  if (!(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}
static inline int check_nt_tc_fused(const void* boards, const void* aux, const void* weights, const void* acc, int64_t B,
                                    int64_t steps, double eps, double lr, double gamma, const void* status) {
  if (int e = check_batch(B, 4)) return e;
  if (!boards || !aux || !weights || !acc || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux) || !aligned16(weights) || !aligned16(acc)) return Q2048_ERR_ALIGN;
  if (nt_tc_overlap(weights, acc)) return Q2048_ERR_RANGE;
  if (steps < 0 || steps > (1 << 30)) return Q2048_ERR_SIZE;
  if (!(eps >= 0.0 && eps <= 1.0) || !(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}

// The synchronous batch step of the network (q2048_nt_sync_*): the checks of the q2048_nt_* counterparts in their
// order, `acc` (then `pend`) directly after `weights` in the NULL and in the alignment list, and after the alignment
// checks two of their own: B <= 2^20 (the bound that keeps every sum exact), and V (256 MiB) and acc (1 GiB) may not
// overlap.
static inline bool nt_sync_overlap(const void* weights, const void* acc) {
  const uintptr_t w0 = reinterpret_cast<uintptr_t>(weights), a0 = reinterpret_cast<uintptr_t>(acc);
  const uintptr_t w1 = w0 + ((uintptr_t)1 << 28), a1 = a0 + ((uintptr_t)1 << 30);
  return a0 < w1 && w0 < a1;
}
static inline int check_nt_sync_update(const void* weights, const void* acc, const void* boards_s, const void* actions,
                                       const void* boards_s2, const void* done, int64_t B, double lr, double gamma,
                                       const void* status) {
  if (int e = check_batch(B, 4)) return e;
  if (!weights || !acc || !boards_s || !actions || !boards_s2 || !done || !status) return Q2048_ERR_NULL;
  if (!aligned16(weights) || !aligned16(acc) || !aligned16(boards_s) || !aligned16(boards_s2)) return Q2048_ERR_ALIGN;
  if (B > ((int64_t)1 << 20) || nt_sync_overlap(weights, acc)) return Q2048_ERR_RANGE;
  if (!(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}
static inline int check_nt_sync_fused(const void* boards, const void* aux, const void* weights, const void* acc,
                                      const void* pend, int64_t B, int64_t steps, double eps, double lr, double gamma,
                                      const void* status) {
  if (int e = check_batch(B, 4)) return e;
  if (!boards || !aux || !weights || !acc || !pend || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux) || !aligned16(weights) || !aligned16(acc) || !aligned16(pend))
    return Q2048_ERR_ALIGN;
  if (B > ((int64_t)1 << 20) || nt_sync_overlap(weights, acc)) return Q2048_ERR_RANGE;
  if (steps < 0 || steps > (1 << 30)) return Q2048_ERR_SIZE;
  if (!(eps >= 0.0 && eps <= 1.0) || !(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}

// TD(lambda) for the network (q2048_nt_lambda_*): the checks of the q2048_nt_* counterparts in their order, `trace`
// directly after `weights` in the NULL list (unless h == 0: no trace is touched) and in the alignment list, and h and
// lambda with the scalars, last.  q2048_nt_choose_ex checks as q2048_nt_choose does: `explored` may be NULL.
static inline bool nt_lambda_ok(double lambda, int h) {
  return h >= 0 && h <= 3 && lambda >= 0.0 && lambda <= 1.0;          // (a NaN fails both comparisons)
}
static inline int check_nt_lambda_update(const void* weights, const void* trace, const void* boards_s,
                                         const void* actions, const void* boards_s2, const void* done, int64_t B,
                                         double lr, double gamma, double lambda, int h, const void* status) {
  if (int e = check_batch(B, 4)) return e;
  if (!weights || (!trace && h != 0) || !boards_s || !actions || !boards_s2 || !done || !status) return Q2048_ERR_NULL;
  if (!aligned16(weights) || !aligned16(trace) || !aligned16(boards_s) || !aligned16(boards_s2)) return Q2048_ERR_ALIGN;
  if (!(lr == lr) || !(gamma == gamma) || !nt_lambda_ok(lambda, h)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}
static inline int check_nt_lambda_fused(const void* boards, const void* aux, const void* weights, const void* trace,
                                        int64_t B, int64_t steps, double eps, double lr, double gamma, double lambda,
                                        int h, const void* status) {
  if (int e = check_batch(B, 4)) return e;
  if (!boards || !aux || !weights || (!trace && h != 0) || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux) || !aligned16(weights) || !aligned16(trace)) return Q2048_ERR_ALIGN;
  if (steps < 0 || steps > (1 << 30)) return Q2048_ERR_SIZE;
  if (!(eps >= 0.0 && eps <= 1.0) || !(lr == lr) || !(gamma == gamma) || !nt_lambda_ok(lambda, h)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}

// The searched row of both afterstate families (q2048_{av,nt}_search_*): the checks of q2048_{av,nt}_lookup and
// q2048_{av,nt}_play_rollout, in their order, with their codes; the legality mask is one more required pointer.
static inline int check_search_lookup(const void* weights, const void* boards, int64_t B, const void* q_out,
                                      const void* legal_out) {
  if (int e = check_batch(B, 4)) return e;
  if (!weights || !boards || !q_out || !legal_out) return Q2048_ERR_NULL;
  if (!aligned16(weights) || !aligned16(boards) || !aligned16(q_out)) return Q2048_ERR_ALIGN;
  return Q2048_OK;
}
static inline int check_search_play(const void* boards, const void* aux, const void* weights, int64_t B, int64_t steps,
                                    double eps, uint32_t flags, const void* status) {
  return check_av_play(boards, aux, weights, B, steps, eps, flags, status);
}
// The same with a search depth (q2048_{av,nt}_search_*_depth): the depth first -- 1 or 2, anything else is
// Q2048_ERR_RANGE whatever the other arguments are -- then the depth-1 counterpart's checks, in its order, with its codes.
static inline int check_search_lookup_depth(const void* weights, const void* boards, int64_t B, int depth,
                                            const void* q_out, const void* legal_out) {
  if (depth != 1 && depth != 2) return Q2048_ERR_RANGE;
  return check_search_lookup(weights, boards, B, q_out, legal_out);
}
static inline int check_search_play_depth(const void* boards, const void* aux, const void* weights, int64_t B,
                                          int64_t steps, int depth, double eps, uint32_t flags, const void* status) {
  if (depth != 1 && depth != 2) return Q2048_ERR_RANGE;
  return check_search_play(boards, aux, weights, B, steps, eps, flags, status);
}

// The staged network (q2048_nts_*): the stage spec first -- a malformed one is Q2048_ERR_RANGE whatever the other
// arguments are, as the depth is -- then the checks of the q2048_nt_* counterpart, in its order, with its codes.
// (What a well-formed spec is, and its S, are written in q2048_core.hpp: nts_spec_ok, nts_count.)
static inline int check_nts_spec(uint32_t stages) { return nts_spec_ok(stages) ? Q2048_OK : Q2048_ERR_RANGE; }
static inline int check_nts_value(const void* weights, uint32_t stages, const void* boards, int64_t B, const void* v_out) {
  if (int e = check_nts_spec(stages)) return e;
  return check_nt_value(weights, boards, B, v_out);
}
static inline int check_nts_lookup(const void* weights, uint32_t stages, const void* boards, int64_t B, const void* q_out) {
  if (int e = check_nts_spec(stages)) return e;
  return check_nt_lookup(weights, boards, B, q_out);
}
static inline int check_nts_choose(const void* weights, uint32_t stages, const void* boards, int64_t B, double eps,
                                   const void* actions) {
  if (int e = check_nts_spec(stages)) return e;
  return check_nt_choose(weights, boards, B, eps, actions);
}
static inline int check_nts_update(const void* weights, uint32_t stages, const void* boards_s, const void* actions,
                                   const void* boards_s2, const void* done, int64_t B, double lr, double gamma,
                                   const void* status) {
  if (int e = check_nts_spec(stages)) return e;
  return check_nt_update(weights, boards_s, actions, boards_s2, done, B, lr, gamma, status);
}
static inline int check_nts_fused(const void* boards, const void* aux, const void* weights, uint32_t stages, int64_t B,
                                  int64_t steps, double eps, double lr, double gamma, const void* status) {
  if (int e = check_nts_spec(stages)) return e;
  return check_nt_fused(boards, aux, weights, B, steps, eps, lr, gamma, status);
}
static inline int check_nts_play(const void* boards, const void* aux, const void* weights, uint32_t stages, int64_t B,
                                 int64_t steps, double eps, uint32_t flags, const void* status) {
  if (int e = check_nts_spec(stages)) return e;
  return check_nt_play(boards, aux, weights, B, steps, eps, flags, status);
}
static inline int check_nts_search_lookup_depth(const void* weights, uint32_t stages, const void* boards, int64_t B,
                                                int depth, const void* q_out, const void* legal_out) {
  if (int e = check_nts_spec(stages)) return e;
  return check_search_lookup_depth(weights, boards, B, depth, q_out, legal_out);
}
static inline int check_nts_search_play_depth(const void* boards, const void* aux, const void* weights, uint32_t stages,
                                              int64_t B, int64_t steps, int depth, double eps, uint32_t flags,
                                              const void* status) {
  if (int e = check_nts_spec(stages)) return e;
  return check_search_play_depth(boards, aux, weights, B, steps, depth, eps, flags, status);
}
// Carousel shaping (q2048_car_*): the spec, NULL, alignment (16 bytes; counts 8), then the sizes and the scalars of
// q2048_nts_fused_rollout.  A ring above 2^32 records is a size error: the slot of a restart is drawn from 32 bits.
static inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
static inline int check_car_fused(const void* boards, const void* aux, const void* weights, uint32_t stages,
                                  const void* pool, const void* counts, const void* fresh, int64_t P, int64_t B,
                                  int64_t steps, double eps, double lr, double gamma, const void* status) {
  if (int e = check_nts_spec(stages)) return e;
  if (!boards || !aux || !weights || !pool || !counts || !fresh || !status) return Q2048_ERR_NULL;
  if (!aligned16(boards) || !aligned16(aux) || !aligned16(weights) || !aligned16(pool) || !aligned16(fresh) ||
      !aligned8(counts))
    return Q2048_ERR_ALIGN;
  if (P < 1 || P > kCarMaxRing) return Q2048_ERR_SIZE;
  if (int e = check_batch(B, 4)) return e;
  if (steps < 0 || steps > (1 << 30)) return Q2048_ERR_SIZE;
  if (!(eps >= 0.0 && eps <= 1.0) || !(lr == lr) || !(gamma == gamma)) return Q2048_ERR_RANGE;
  return Q2048_OK;
}
static inline int check_car_commit(const void* pool, const void* counts, const void* fresh, uint32_t stages, int64_t P,
                                   int64_t B) {
  if (int e = check_nts_spec(stages)) return e;
  if (!pool || !counts || !fresh) return Q2048_ERR_NULL;
  if (!aligned16(pool) || !aligned16(fresh) || !aligned8(counts)) return Q2048_ERR_ALIGN;
  if (P < 1 || P > kCarMaxRing) return Q2048_ERR_SIZE;
  return check_batch(B, 4);
}
// q2048_nts_promote: the spec, NULL, alignment, then the two stage numbers (from == to, or either >= S)
static inline int check_nts_promote(const void* weights, uint32_t stages, int from, int to) {
  if (int e = check_nts_spec(stages)) return e;
  if (!weights) return Q2048_ERR_NULL;
  if (!aligned16(weights)) return Q2048_ERR_ALIGN;
  const int S = (int)nts_count(stages);
  if (from < 0 || to < 0 || from >= S || to >= S || from == to) return Q2048_ERR_RANGE;
  return Q2048_OK;
}

// q2048_strerror
static inline const char* error_text(int code) {
  switch (code) {
    case Q2048_OK: return "ok";
    case Q2048_ERR_NULL: return "a required pointer is NULL";
    case Q2048_ERR_SIZE: return "size out of range (batch, steps, cap_log2 or key_words)";
    case Q2048_ERR_ALIGN: return "boards/aux/table must be 16-byte aligned";
    case Q2048_ERR_UNSUPPORTED: return "unsupported here (board side other than 4 or 5, or an entry point this library or geometry does not have)";
    case Q2048_ERR_LAUNCH: return "HIP launch failed";
    case Q2048_ERR_RANGE: return "scalar out of range (eps in [0,1], lr and gamma finite, search depth 1 or 2)";
    case Q2048_ERR_FLAGS: return "flag bits this entry point does not take";
    case Q2048_ERR_ALLOC: return "device memory could not be reserved, created or mapped";
    case Q2048_ERR_VERIFY: return "a table failed its self-check (a fresh table not all zeros, or rows lost while growing)";
    case Q2048_ERR_BUSY: return "the table already takes part in a growth (finish or abort that one first)";
    case Q2048_PENDING: return "still working (not an error)";
    default: return "unknown error";
  }
}

}  // namespace q2048
