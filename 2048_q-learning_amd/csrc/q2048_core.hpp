// q2048_core.hpp -- per-lane arithmetic of the batched 2048 Q-learning step (4x4 board).
//
// One board lives in one lane: 16 x uint8 log2 tiles = four 32-bit row words in VGPRs
// (word r = row r, byte c = column c; 0 = empty, k = tile 2^k).  Everything here is
// register-only integer/fp arithmetic with no memory access, written once and compiled
//   * by hipcc for gfx950 (the kernels in q2048_kernels.hip), and
//   * by g++ for tests/hostcheck, which checks these exact functions against the CPU oracle
//     exhaustively before anything runs on a GPU.
// It is NOT a CPU fallback: the host instantiation serves tests/hostcheck and the explicit device "cpu"
// (q2048_host.cpp), which is built from these functions and nothing else.
// It also holds the one definition of the Q-table's format ("THE TABLE'S FORMAT" below, keys in q2048_core5.hpp).
//
// What each function replaces in the reference (paths under QLearningBase/):
//   move()            environment/Game2048_env.py:22-63  (rotate/move_left/rotate back)
//   spawn()           :16-20   add_number
//   game_over()       :65-75   closed form of the four trial moves
//   env_step()        :97-129  step + calculate_reward :136-184 + update_and_normalize :197-205
//   reset_board()     :11-14, :187-191
//   pack_key()        Agent/main.py:82,94  tuple(map(tuple, state))
//   eps_greedy()      Agent/main.py:34-38
//   td_value()        Agent/main.py:40-43
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#define Q_HD __host__ __device__ __forceinline__
#else
#define Q_HD inline
#endif

#include "q2048_luts.inc"

namespace q2048 {

// ------------------------------------------------------------------------------------------
// counter RNG: Philox4x32-10, counter = (env_id lo, env_id hi, step counter, stream),
// key = (seed lo, seed hi).  One call serves one env step:
//   x[0] epsilon test, x[1] random action, x[2] spawn cell, x[3] spawn value.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kStreamStep = 0u, kStreamReset = 1u, kStreamOver = 2u;

struct Draws { uint32_t x0, x1, x2, x3; };

// (Q2048_PHILOX_ROUNDS: measurement builds only -- tools/archive/sessions/r04_philox7.sh times the rollouts with
// Philox4x32-7, the smallest variant that passes BigCrush, against the 10 rounds of the draw contract.)
#ifndef Q2048_PHILOX_ROUNDS
#define Q2048_PHILOX_ROUNDS 10
#endif
// one round on the counter words; the caller steps the key (Weyl sequence) between rounds
Q_HD void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
  c1 = (uint32_t)p1;
  c3 = (uint32_t)p0;
  c0 = n0;
  c2 = n2;
}
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

Q_HD Draws philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                         uint32_t k1) {
#pragma unroll
  for (int r = 0; r < Q2048_PHILOX_ROUNDS; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return Draws{c0, c1, c2, c3};
}

// THE DEFINITION of the draws of (seed, env id, counter, stream); everything below must equal it
Q_HD Draws draws(uint64_t seed, uint64_t env_id, uint32_t ctr, uint32_t stream) {
  return philox4x32_10((uint32_t)env_id, (uint32_t)(env_id >> 32), ctr, stream, (uint32_t)seed,
                       (uint32_t)(seed >> 32));
}

// The same draws for a loop over the counter: of the four counter words only c2 = ctr changes from step to
// step, so round 1's 0xD2511F53 * c0 and -- its high half being all of round 2's c2 -- round 2's
// 0xCD9E8D57 * c2 are the same on every step.  draws_prepare does those two products once per env,
// draws_at the other 2 * ROUNDS - 2 (the one on ctr alone is the same for every env of a launch: on the
// device it is scalar arithmetic).  draws_at(draws_prepare(seed, id, stream), ctr) == draws(seed, id, ctr, stream).
static_assert(Q2048_PHILOX_ROUNDS >= 2, "draws_prepare folds the first two rounds");
struct DrawPrep {
  uint32_t a;        // c1 ^ k0: round 1's c0 but for hi(M1 * ctr)
  uint32_t b;        // hi(M1 * n2) ^ (k0 + W0): round 2's c0 but for lo(M1 * ctr)
  uint32_t c;        // lo(M0 * c0) ^ (k1 + W1): round 2's c2 but for hi(M0 * round 1's c0)
  uint32_t d;        // lo(M1 * n2): c1 after round 2
  uint32_t k0, k1;   // the key after two rounds
};
Q_HD DrawPrep draws_prepare(uint64_t seed, uint64_t env_id, uint32_t stream) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  const uint64_t p0 = (uint64_t)0xD2511F53u * (uint32_t)env_id;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ stream ^ k1;          // round 1's c2
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * n2;
  return DrawPrep{(uint32_t)(env_id >> 32) ^ k0, (uint32_t)(p1 >> 32) ^ (k0 + kPhiloxW0),
                  (uint32_t)p0 ^ (k1 + kPhiloxW1), (uint32_t)p1, k0 + 2u * kPhiloxW0, k1 + 2u * kPhiloxW1};
}
Q_HD Draws draws_at(const DrawPrep& p, uint32_t ctr) {
  const uint64_t q1 = (uint64_t)0xCD9E8D57u * ctr;                  // round 1, the counter's product
  const uint64_t q0 = (uint64_t)0xD2511F53u * ((uint32_t)(q1 >> 32) ^ p.a);   // round 2
  uint32_t c0 = p.b ^ (uint32_t)q1, c1 = p.d, c2 = (uint32_t)(q0 >> 32) ^ p.c, c3 = (uint32_t)q0;
  uint32_t k0 = p.k0, k1 = p.k1;
#pragma unroll
  for (int r = 2; r < Q2048_PHILOX_ROUNDS; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return Draws{c0, c1, c2, c3};
}

// draw -> decision (DESIGN.md "draw contract"; the reference call each replaces is cited there)
Q_HD double draw_uniform(uint32_t x) { return (double)x * (1.0 / 4294967296.0); }
Q_HD int draw_action(uint32_t x) { return (int)(x >> 30); }
Q_HD uint32_t draw_index(uint32_t x, uint32_t n) { return (uint32_t)(((uint64_t)x * n) >> 32); }
// not (random() < 0.9) (Game2048_env.py:20): x / 2^32 < 0.9 (the double nearest 0.9) holds exactly for
// x <= 3865470566 (0.9 * 2^32 = 3865470566.4), so the test is an integer compare
Q_HD bool draw_is_four(uint32_t x) { return x >= 3865470567u; }

// ------------------------------------------------------------------------------------------
// SWAR helpers on four tile bytes per word.  Every tile byte is <= 0x7f (log2 <= 17 on 4x4).
// ------------------------------------------------------------------------------------------
Q_HD uint32_t nz80(uint32_t x) { return (x + 0x7f7f7f7fu) & 0x80808080u; }       // 0x80 per byte != 0
Q_HD uint32_t z80(uint32_t x) { return ~(x + 0x7f7f7f7fu) & 0x80808080u; }       // 0x80 per byte == 0
Q_HD uint32_t fill80(uint32_t m) { return (m << 1) - (m >> 7); }                 // 0x80 -> 0xff
// 0x80 -> 0x7f: as good a select mask as 0xff between words whose bytes are all <= 0x7f (bit 7 is
// 0 on both sides), one instruction less
Q_HD uint32_t fill7f(uint32_t m) { return m - (m >> 7); }
Q_HD uint32_t bsel(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }

struct Board { uint32_t r0, r1, r2, r3; };

Q_HD bool operator==(const Board& a, const Board& b) {
  return ((a.r0 ^ b.r0) | (a.r1 ^ b.r1) | (a.r2 ^ b.r2) | (a.r3 ^ b.r3)) == 0;
}
Q_HD void clear(Board& b) { b = Board{0u, 0u, 0u, 0u}; }

// 4x4 byte transpose: out word j = column j (byte i = row i)
Q_HD Board transpose(const Board& b) {
  const uint32_t a0 = (b.r0 & 0x00ff00ffu) | ((b.r1 & 0x00ff00ffu) << 8);
  const uint32_t a1 = ((b.r0 >> 8) & 0x00ff00ffu) | (b.r1 & 0xff00ff00u);
  const uint32_t b0 = (b.r2 & 0x00ff00ffu) | ((b.r3 & 0x00ff00ffu) << 8);
  const uint32_t b1 = ((b.r2 >> 8) & 0x00ff00ffu) | (b.r3 & 0xff00ff00u);
  return Board{(a0 & 0xffffu) | (b0 << 16), (a1 & 0xffffu) | (b1 << 16),
               (a0 >> 16) | (b0 & 0xffff0000u), (a1 >> 16) | (b1 & 0xffff0000u)};
}

// sum over the four bytes b of (b ? 2^b : 0); merged tiles are >= 2 so bit 0 never counts
Q_HD uint32_t pow2_sum(uint32_t v) {
  return (((1u << (v & 0xffu)) & ~1u) + ((1u << ((v >> 8) & 0xffu)) & ~1u)) +
         (((1u << ((v >> 16) & 0xffu)) & ~1u) + ((1u << (v >> 24)) & ~1u));
}

// Slide/merge four lines at once.  c_j holds cell j (counted from the edge the tiles move
// to) of each of the four lines, one line per byte.  Restates move_left
// (Game2048_env.py:25-44): compress, then one left-to-right merge pass without cascade.
Q_HD uint32_t slide_lines(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3) {
  uint32_t z;
  // compress (:26): pull cells towards c0 while the head cell is empty
#pragma unroll
  for (int rep = 0; rep < 3; ++rep) {
    z = fill7f(z80(c0));
    c0 = bsel(z, c1, c0); c1 = bsel(z, c2, c1); c2 = bsel(z, c3, c2); c3 &= ~z;
  }
#pragma unroll
  for (int rep = 0; rep < 2; ++rep) {
    z = fill7f(z80(c1));
    c1 = bsel(z, c2, c1); c2 = bsel(z, c3, c2); c3 &= ~z;
  }
  z = fill7f(z80(c2));
  c2 = bsel(z, c3, c2); c3 &= ~z;
  // merge (:29-40): pair (0,1), then the next unmerged pair, never re-merging a result
  uint32_t e = z80(c0 ^ c1) & nz80(c0);
  uint32_t m = fill7f(e);
  c0 += e >> 7;
  const uint32_t s_a = c0 & m;
  c1 = bsel(m, c2, c1); c2 = bsel(m, c3, c2); c3 &= ~m;
  e = z80(c1 ^ c2) & nz80(c1);
  m = fill7f(e);
  c1 += e >> 7;
  const uint32_t s_b = c1 & m;
  c2 = bsel(m, c3, c2); c3 &= ~m;
  e = z80(c2 ^ c3) & nz80(c2);
  m = fill7f(e);
  c2 += e >> 7;
  c3 &= ~m;
  const uint32_t s_c = c2 & m;  // a line that merged at (2,3) merged nowhere else
  return pow2_sum(s_a | s_c) + pow2_sum(s_b);  // score += merged value (:36)
}

// Game2048.move without the spawn (:51-60).  action: 0 left, 1 up, 2 right, 3 down (:54).
// Direction-agnostic: pick the four "cell j of every line" words by select, no branch.
Q_HD bool move(Board& b, int action, uint32_t& score) {
  const bool horiz = (action & 1) == 0;  // lines are rows: take columns as cell words
  const bool rev = (action & 2) != 0;    // right / down: cell 0 is the far edge
  const Board t = transpose(b);
  const uint32_t p0 = horiz ? t.r0 : b.r0, p1 = horiz ? t.r1 : b.r1;
  const uint32_t p2 = horiz ? t.r2 : b.r2, p3 = horiz ? t.r3 : b.r3;
  uint32_t c0 = rev ? p3 : p0, c1 = rev ? p2 : p1, c2 = rev ? p1 : p2, c3 = rev ? p0 : p3;
  const uint32_t o0 = c0, o1 = c1, o2 = c2, o3 = c3;
  score = slide_lines(c0, c1, c2, c3);
  const bool moved = ((c0 ^ o0) | (c1 ^ o1) | (c2 ^ o2) | (c3 ^ o3)) != 0;  // :38,42-43
  const Board q{rev ? c3 : c0, rev ? c2 : c1, rev ? c1 : c2, rev ? c0 : c3};
  const Board qt = transpose(q);
  b.r0 = horiz ? qt.r0 : q.r0; b.r1 = horiz ? qt.r1 : q.r1;
  b.r2 = horiz ? qt.r2 : q.r2; b.r3 = horiz ? qt.r3 : q.r3;
  return moved;
}

// 16-bit mask of empty cells, bit = row-major cell index (np.where order, :17)
Q_HD uint32_t movemask(uint32_t m80) { return (((m80 >> 7) * 0x01020408u) >> 24) & 0xfu; }
Q_HD uint32_t empty_mask(const Board& b) {
  return movemask(z80(b.r0)) | (movemask(z80(b.r1)) << 4) | (movemask(z80(b.r2)) << 8) |
         (movemask(z80(b.r3)) << 12);
}

Q_HD uint32_t popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }

// index of the k-th (0-based) set bit of a 16-bit mask, k < popcount(mask)
Q_HD uint32_t kth_set_bit16(uint32_t mask, uint32_t k) {
  uint32_t pos = 0, c;
  bool ge;
  c = popc(mask & 0xffu); ge = k >= c; k -= ge ? c : 0u; pos += ge ? 8u : 0u; mask >>= ge ? 8u : 0u;
  c = popc(mask & 0xfu);  ge = k >= c; k -= ge ? c : 0u; pos += ge ? 4u : 0u; mask >>= ge ? 4u : 0u;
  c = popc(mask & 0x3u);  ge = k >= c; k -= ge ? c : 0u; pos += ge ? 2u : 0u; mask >>= ge ? 2u : 0u;
  c = mask & 1u;          ge = k >= c; pos += ge ? 1u : 0u;
  return pos;
}

Q_HD void put_cell(Board& b, uint32_t pos, uint32_t v) {
  const uint32_t w = v << ((pos & 3u) * 8u), row = pos >> 2;
  b.r0 |= row == 0u ? w : 0u; b.r1 |= row == 1u ? w : 0u;
  b.r2 |= row == 2u ? w : 0u; b.r3 |= row == 3u ? w : 0u;
}

// Game2048.add_number (:16-20): k-th empty cell in row-major order gets 2 (p=.9) or 4
Q_HD void spawn(Board& b, uint32_t draw_pos, uint32_t draw_val) {
  const uint32_t em = empty_mask(b), n = popc(em);
  if (n == 0u) return;  // :18
  put_cell(b, kth_set_bit16(em, draw_index(draw_pos, n)), draw_is_four(draw_val) ? 2u : 1u);
}

// Game2048.is_game_over (:65-75) in closed form: full board and no equal neighbours.  On a
// full board a trial move changes something iff some line holds an equal adjacent pair.
Q_HD bool game_over(const Board& b) {
  const uint32_t empties = z80(b.r0) | z80(b.r1) | z80(b.r2) | z80(b.r3);
  const uint32_t vert = z80(b.r0 ^ b.r1) | z80(b.r1 ^ b.r2) | z80(b.r2 ^ b.r3);
  const uint32_t horz = (z80(b.r0 ^ (b.r0 >> 8)) | z80(b.r1 ^ (b.r1 >> 8)) |
                         z80(b.r2 ^ (b.r2 >> 8)) | z80(b.r3 ^ (b.r3 >> 8))) & 0x00808080u;
  return (empties | vert | horz) == 0u;
}

Q_HD uint32_t bytemax(uint32_t a, uint32_t b) {  // per-byte max, bytes <= 0x7f
  const uint32_t m = fill7f(((a | 0x80808080u) - b) & 0x80808080u);
  return bsel(m, a, b);
}
Q_HD uint32_t max_log2(const Board& b) {  // np.max(board) (:100), as log2
  uint32_t x = bytemax(bytemax(b.r0, b.r1), bytemax(b.r2, b.r3));
  x = bytemax(x, x >> 16);
  x = bytemax(x, x >> 8);
  return x & 0xffu;
}

// ------------------------------------------------------------------------------------------
// per-env shaping state (Game2048_env.__init__, :81-95) -- 16 bytes, one dwordx4 per lane
// ------------------------------------------------------------------------------------------
struct Aux {
  int32_t score;        // env.score (:84), reset per episode (:190)
  float ep_return;      // total_reward of Agent/main.py:84,101
  uint8_t prev_max;     // log2(previous_max) (:87), survives reset()
  uint8_t cons_action;  // consecutive_action (:92), 0xFF = None, survives reset()
  uint16_t cons_count;  // consecutive_count (:93), saturating, survives reset()
  uint32_t episode;     // resets so far = counter of the reset draws
};
constexpr uint8_t kNoAction = 0xFFu;
constexpr uint32_t kConsCountSat = 60000u;  // every count > 100 behaves alike (:121-125)

Q_HD Aux aux_init() { return Aux{0, 0.0f, 1, kNoAction, 0, 0u}; }

Q_HD double lut_pow12(uint32_t L) { constexpr double t[32] = Q2048_POW12; return t[L & 31u]; }
Q_HD double lut_log2p1(uint32_t L) { constexpr double t[32] = Q2048_LOG2P1; return t[L & 31u]; }
Q_HD double lut_stall(uint32_t k) { constexpr double t[32] = Q2048_STALL; return t[k < 31u ? k : 31u]; }


// WHERE the five tables are read from.  Indexed per lane, a constexpr array becomes a vector load from constant
// memory in the middle of the step -- on the device that is the address path of the table requests, and the wait
// for its answer also waits for every table request still in flight.  The fused rollout therefore stages one
// LutImage per workgroup in LDS and steps through ImageLuts; ConstLuts (the arrays above) is the definition and
// the default of every function below.  Both are initialised from the same generated lists: equal bit for bit.
struct LutImage { double pow12[32], log2p1[32], stall[32], log2_inv[64], log2_lg[64]; };
#define Q2048_LUT_IMAGE { Q2048_POW12, Q2048_LOG2P1, Q2048_STALL, Q2048_LOG2_INV, Q2048_LOG2_LG }
constexpr int kLutImageDoubles = (int)(sizeof(LutImage) / sizeof(double));   // 224: 1792 bytes
struct ConstLuts {
  Q_HD double pow12(uint32_t L) const { return lut_pow12(L); }
  Q_HD double log2p1(uint32_t L) const { return lut_log2p1(L); }
  Q_HD double stall(uint32_t k) const { return lut_stall(k); }
  Q_HD double log2_inv(uint32_t j) const { constexpr double t[64] = Q2048_LOG2_INV; return t[j & 63u]; }
  Q_HD double log2_lg(uint32_t j) const { constexpr double t[64] = Q2048_LOG2_LG; return t[j & 63u]; }
};
struct ImageLuts {
  const LutImage* im;
  Q_HD double pow12(uint32_t L) const { return im->pow12[L & 31u]; }
  Q_HD double log2p1(uint32_t L) const { return im->log2p1[L & 31u]; }
  Q_HD double stall(uint32_t k) const { return im->stall[k < 31u ? k : 31u]; }
  Q_HD double log2_inv(uint32_t j) const { return im->log2_inv[j & 63u]; }
  Q_HD double log2_lg(uint32_t j) const { return im->log2_lg[j & 63u]; }
};

Q_HD uint64_t f64_bits(double d) { union { double d; uint64_t u; } c; c.d = d; return c.u; }
Q_HD double bits_f64(uint64_t u) { union { double d; uint64_t u; } c; c.u = u; return c.d; }

// log2(x) for finite x >= 1, relative error < 2^-46 (checked against libm in
// tests/test_core_host.py): ~20 instructions instead of the math library's ~110.  The reward is
// stored as float32, so this is >20 bits more than the rounding it feeds.
//   x = m * 2^e, m in [1, 2);  j = top 6 mantissa bits;  r = m * inv[j] - 1, |r| <= 2^-7;
//   log2(x) = e + lg[j] + r * (a1 + r * (a2 + ... + r * a6)),  lg[j] = -log2(inv[j]) exactly.
template <class LutT = ConstLuts>
Q_HD double log2_ge1(double x, const LutT& lut = LutT()) {
  constexpr double a[6] = Q2048_LOG2_COEF;
  const uint64_t u = f64_bits(x);
  const int e = (int)(u >> 52) - 1023;
  const uint32_t j = (uint32_t)(u >> 46) & 63u;
  const double m = bits_f64((u & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
  const double r = fma(m, lut.log2_inv(j), -1.0);
  double p = fma(r, a[5], a[4]);
  p = fma(r, p, a[3]);
  p = fma(r, p, a[2]);
  p = fma(r, p, a[1]);
  p = fma(r, p, a[0]);
  return fma(r, p, (double)e + lut.log2_lg(j));
}

// update_and_normalize (:197-205); both log2 arguments are >= 1
// One logarithm serves both signs: |r - 1| for r < 0 is |r| + 1, the same double (rounding is
// symmetric), and r + 1 is |r| + 1 for r >= 0 (-0.0 included).
template <class LutT = ConstLuts>
Q_HD double normalize_reward(double r, const LutT& lut = LutT()) {
  const double v = fmin(log2_ge1(fabs(r) + 1.0, lut), 10.0);
  return r >= 0 ? v : -v;
}

// calculate_reward (:136-184); L = log2(max tile), prev = log2(previous_max), both integers
template <class LutT = ConstLuts>
Q_HD double calculate_reward(uint32_t score, bool valid, bool over, uint32_t L, uint8_t& prev,
                             const LutT& lut = LutT()) {
  L = L < 1u ? 1u : L;                                   // :141
  const double cl = (double)L;                           // :144
  double bonus = 0.0, r;
  if (L > prev) {                                        // :148
    bonus = (cl - (double)prev) * lut.pow12(L);          // :149
    prev = (uint8_t)L;                                   // :150
  }
  if (!valid) {
    if (over) {
      if (L >= 9u && L <= 11u) r = bonus + lut.pow12(L); // :156-158
      else r = 0.0 - lut.log2p1(L);                      // :160
    } else {
      r = 0.0 - 0.1 * cl;                                // :164
    }
  } else {
    r = (double)score;                                   // :168
    if (bonus > 0) r += bonus;                           // :171-172
    else r += cl * 0.05;                                 // :173-174
    if (L >= 9u) r += lut.pow12(L) * 2;                  // :176-177
  }
  return normalize_reward(r, lut);                          // :181
}

struct StepOut {
  float reward;      // reward rounded to f32 (the TD update consumes exactly this value)
  double reward64;   // before rounding, for parity reports
  uint32_t score;    // merge score of this move
  uint8_t done, max_log2, valid;
};

// the spawn of a valid move (Game2048_env.py:61-62), then is_game_over (:99); the 5x5 board has its
// own version that counts the empty cells once for both
template <class BoardT>
Q_HD bool spawn_then_over(BoardT& b, bool valid, uint32_t x_pos, uint32_t x_val) {
  if (valid) spawn(b, x_pos, x_val);
  return game_over(b);
}

// Game2048_env.step (:97-129) for one lane.  x_pos/x_val are the spawn draws.  BoardT is the
// 4x4 Board above or the 5x5 Board5 of q2048_core5.hpp (same functions, overloaded).
template <class BoardT, class LutT = ConstLuts>
Q_HD StepOut env_step(BoardT& b, Aux& a, int action, uint32_t x_pos, uint32_t x_val, const LutT& lut = LutT()) {
  StepOut o;
  uint32_t score;
  const bool valid = move(b, action, score);                            // :98
  const bool over = spawn_then_over(b, valid, x_pos, x_val);            // :61-62, :99
  const uint32_t mx = max_log2(b);                                      // :100
  a.score += (int32_t)score;                                            // :104
  double r = calculate_reward(score, valid, over, mx, a.prev_max, lut); // :107
  uint32_t cnt = a.cons_count;
  if ((uint8_t)action == a.cons_action) {                               // :110
    cnt = cnt + 1u < kConsCountSat ? cnt + 1u : kConsCountSat;          // :111
  } else {
    a.cons_action = (uint8_t)action;                                    // :113
    cnt = 1u;                                                           // :114-115
  }
  a.cons_count = (uint16_t)cnt;
  bool done = !valid && over;                                           // :117-118
  if (cnt > 10u) {                                                      // :121
    if (cnt > 100u) done = true;                                        // :122-123
    r += lut.stall(cnt - 10u);                                          // :124-127
  }
  o.reward64 = r;
  o.reward = (float)r;
  a.ep_return += o.reward;
  o.score = score;
  o.done = done;
  o.max_log2 = (uint8_t)mx;
  o.valid = valid;
  return o;
}

// Env profiles (template parameter ENV of the kernels, from Q2048_FLAG_ENV_DQN / _RESET_SHAPING / _PLAY_ONLY):
//   kEnvDqn           step of the DQN path's env, Deep_QLearning/environment/
//                     Game2048_nopenalty_env.py:106-138, instead of Game2048_env.step
//   kEnvResetShaping  resets also restore previous_max and the consecutive-action state
//                     (SURVEY 7.8 opt-in; Game2048_env.reset, :187-191, leaves them alone)
//   kEnvPlayOnly      (fused rollout only) no learner: the table is neither read nor written
constexpr int kEnvDqn = 1, kEnvResetShaping = 2, kEnvPlayOnly = 4;

// Game2048_nopenalty_env.step (:106-120) with the caller's `env.game.board = next_state`
// (mainDQL_CNN_step2.py:237) folded in: on return b is moved_board.
//   - move works on a copy (:58); is_game_over (:68-78) inspects the board from BEFORE the move:
//     False if it has an empty cell (:70-71); on a full board it makes real moves 0..3 (:72-74) and
//     the first that changes something leaves ITS result, spawn included (draws y_pos, y_val), in
//     moved_board (:75-77) -- that, not the chosen action's move, is what the step returns;
//   - reward = calculate_reward2 (:122-138): -10 for an invalid move while not over, else the
//     chosen move's merge score; done = game_over (:117-118); max tile of moved_board (:109).
template <class BoardT>
Q_HD StepOut env_step_dqn(BoardT& b, Aux& a, int action, uint32_t x_pos, uint32_t x_val,
                          uint32_t y_pos, uint32_t y_val) {
  StepOut o;
  const BoardT pre = b;
  uint32_t score;
  const bool valid = move(b, action, score);                            // :107 -> :53-63
  if (valid) spawn(b, x_pos, x_val);                                    // :64-65
  bool over = false;
  if (empty_mask(pre) == 0u) {                                          // :70
    over = true;
    for (int act = 0; act < 4 && over; ++act) {                         // :72
      BoardT t = pre;                                                   // :58
      uint32_t s2;
      if (move(t, act, s2)) {                                           // :74
        spawn(t, y_pos, y_val);                                         // :64-65
        b = t;
        over = false;                                                   // :75-77
      }
    }
    if (over) b = pre;                      // nothing moved: moved_board is a copy of the board
  }
  const uint32_t mx = max_log2(b);                                      // :109
  a.score += (int32_t)score;                                            // :112
  const double r = (!valid && !over) ? -10.0 : (double)score;           // :125-128
  o.reward64 = r;
  o.reward = (float)r;
  a.ep_return += o.reward;
  o.score = score;
  o.done = over;                                                        // :117-118
  o.max_log2 = (uint8_t)mx;
  o.valid = valid;
  return o;
}

// the step of profile ENV; (y_pos, y_val) are only used by kEnvDqn
template <int ENV, class BoardT, class LutT = ConstLuts>
Q_HD StepOut env_step_profile(BoardT& b, Aux& a, int action, uint32_t x_pos, uint32_t x_val,
                              uint32_t y_pos, uint32_t y_val, const LutT& lut = LutT()) {
  if constexpr ((ENV & kEnvDqn) != 0) return env_step_dqn(b, a, action, x_pos, x_val, y_pos, y_val);
  else return env_step(b, a, action, x_pos, x_val, lut);
}

// Game2048.__init__ (:11-14) / Game2048_env.reset (:187-191): empty board, two spawns,
// score = 0.  previous_max and the consecutive-action state are NOT reset (:187-191).
template <class BoardT>
Q_HD void reset_board(BoardT& b, Aux& a, const Draws& d) {
  clear(b);
  spawn(b, d.x0, d.x1);
  spawn(b, d.x2, d.x3);
  a.score = 0;
  a.ep_return = 0.0f;
}

// env construction (Game2048_env.__init__, :81-95) and the reset that follows a finished
// episode (Agent/main.py:81): the spawn draws are keyed by (env id, episode index)
template <class BoardT>
Q_HD void init_env(BoardT& b, Aux& a, uint64_t seed, uint64_t env_id) {
  a = aux_init();
  reset_board(b, a, draws(seed, env_id, 0u, kStreamReset));
}
template <class BoardT>
Q_HD void begin_episode(BoardT& b, Aux& a, uint64_t seed, uint64_t env_id,
                        bool reset_shaping = false) {
  a.episode += 1u;
  reset_board(b, a, draws(seed, env_id, a.episode, kStreamReset));
  if (reset_shaping) {            // what Game2048_env.__init__ sets (:87, :92-93)
    a.prev_max = 1;
    a.cons_action = kNoAction;
    a.cons_count = 0;
  }
}

// register <-> memory images (little endian): board = 16 bytes, aux = 16 bytes
struct Words4 { uint32_t w0, w1, w2, w3; };
Q_HD uint32_t f32_bits(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }
Q_HD float bits_f32(uint32_t u) { union { float f; uint32_t u; } c; c.u = u; return c.f; }
Q_HD Words4 aux_to_words(const Aux& a) {
  return Words4{(uint32_t)a.score, f32_bits(a.ep_return),
                (uint32_t)a.prev_max | ((uint32_t)a.cons_action << 8) | ((uint32_t)a.cons_count << 16),
                a.episode};
}
Q_HD Aux words_to_aux(const Words4& w) {
  return Aux{(int32_t)w.w0, bits_f32(w.w1), (uint8_t)(w.w2 & 0xffu), (uint8_t)((w.w2 >> 8) & 0xffu),
             (uint16_t)(w.w2 >> 16), w.w3};
}

// ------------------------------------------------------------------------------------------
// agent arithmetic
// ------------------------------------------------------------------------------------------
// state key (Agent/main.py:82): 16 log2 nibbles, cell 0 in the low nibble.  Tiles above 2^15
// do not fit a nibble; `overflow` reports them (the low nibble is used, states alias).
Q_HD uint32_t pack_row(uint32_t x) {
  x &= 0x0f0f0f0fu;
  x = (x | (x >> 4)) & 0x00ff00ffu;
  return (x | (x >> 8)) & 0xffffu;
}
Q_HD uint64_t pack_key(const Board& b, bool& overflow) {
  overflow = ((b.r0 | b.r1 | b.r2 | b.r3) & 0xf0f0f0f0u) != 0u;
  return (uint64_t)(pack_row(b.r0) | (pack_row(b.r1) << 16)) |
         ((uint64_t)(pack_row(b.r2) | (pack_row(b.r3) << 16)) << 32);
}
Q_HD uint32_t unpack_row(uint32_t k) {
  k &= 0xffffu;
  k = (k | (k << 8)) & 0x00ff00ffu;
  return (k | (k << 4)) & 0x0f0f0f0fu;
}
Q_HD Board unpack_key(uint64_t key) {
  return Board{unpack_row((uint32_t)key), unpack_row((uint32_t)(key >> 16)),
               unpack_row((uint32_t)(key >> 32)), unpack_row((uint32_t)(key >> 48))};
}

// ------------------------------------------------------------------------------------------
// SYMMETRY FOLDING (include/q2048.h, Q2048_FLAG_SYMMETRIC): one table row for the eight mirror images of a
// board.  The images of b, in numpy terms:  g = 0..3: np.rot90(b, g);  g = 4..7: np.rot90(np.fliplr(b), g - 4).
// With T = transpose, H = np.fliplr, V = np.flipud these are
//   g:  0 b    1 V(T b)    2 V(H b)    3 H(T b)    4 H b    5 T b    6 V b    7 V(H(T b))
// All of it works on the packed key (cell 4r + c in nibble 4r + c: a row is 16 bits): shifts and masks, no
// memory access.  The canonical image is the one with the smallest key; on a tie the smallest g.
// ------------------------------------------------------------------------------------------
Q_HD uint64_t key_flip_h(uint64_t k) {          // np.fliplr: the four nibbles of every row reversed
  k = ((k & 0x0f0f0f0f0f0f0f0full) << 4) | ((k >> 4) & 0x0f0f0f0f0f0f0f0full);
  return ((k & 0x00ff00ff00ff00ffull) << 8) | ((k >> 8) & 0x00ff00ff00ff00ffull);
}
Q_HD uint64_t key_flip_v(uint64_t k) {          // np.flipud: the four rows reversed
  k = ((k & 0x0000ffff0000ffffull) << 16) | ((k >> 16) & 0x0000ffff0000ffffull);
  return (k << 32) | (k >> 32);
}
Q_HD uint64_t key_transpose(uint64_t k) {       // nibble (r, c) <-> (c, r): 2x2 blocks of nibbles, then of bytes
  const uint64_t a = (k & 0xf0f00f0ff0f00f0full) | ((k & 0x0000f0f00000f0f0ull) << 12) | ((k & 0x0f0f00000f0f0000ull) >> 12);
  return (a & 0xff00ff0000ff00ffull) | ((a & 0x00ff00ff00000000ull) >> 24) | ((a & 0x00000000ff00ff00ull) << 24);
}
struct Canon { uint64_t key; uint32_t g; };     // the canonical image's key and which image it is
Q_HD Canon canonical_key(uint64_t k) {
  const uint64_t t = key_transpose(k), hk = key_flip_h(k), ht = key_flip_h(t);
  const uint64_t cand[8] = {k, key_flip_v(t), key_flip_v(hk), ht, hk, t, key_flip_v(k), key_flip_v(ht)};
  Canon c{k, 0u};
#pragma unroll
  for (uint32_t g = 1; g < 8u; ++g) {           // ascending g, strict <: the smallest g wins a tie
    const bool lt = cand[g] < c.key;
    c.key = lt ? cand[g] : c.key;
    c.g = lt ? g : c.g;
  }
  return c;
}
// image g of a board in bytes (what q2048_canonicalize writes: tiles above 2^15 keep their value)
Q_HD Board board_image(const Board& b, uint32_t g) {
  const Board t = transpose(b);
  Board o = (g & 1u) ? t : b;                                        // g odd: the images of T b
  if ((0x9cu >> g) & 1u)                                             // H for g in {2, 3, 4, 7}
    o = Board{__builtin_bswap32(o.r0), __builtin_bswap32(o.r1), __builtin_bswap32(o.r2), __builtin_bswap32(o.r3)};
  if ((0xc6u >> g) & 1u) o = Board{o.r3, o.r2, o.r1, o.r0};          // V for g in {1, 2, 6, 7}
  return o;
}
// pi_g: move(image_g(b), pi_g(a)) == image_g(move(b, a)) with a = 0 left, 1 up, 2 right, 3 down -- a quarter
// turn counter-clockwise takes "up" to "left", the mirror swaps left and right.  A row stored in the canonical
// frame is read in the env's frame as Q_env[a] = Q_canon[pi_g(a)].
Q_HD int sym_action(uint32_t g, int a) {
  return (int)((g < 4u ? (uint32_t)a - g : 2u - (uint32_t)a - g) & 3u);
}

Q_HD uint64_t mix64(uint64_t h) {
  h *= 0x9E3779B97F4A7C15ull;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 32;
  return h;
}
// independent-learners mode: every env owns private rows of the shared table
Q_HD uint64_t lane_salt(uint64_t env_id) { return mix64(env_id + 0x2048ull) | 1ull; }

// ------------------------------------------------------------------------------------------
// THE TABLE'S FORMAT (q2048_slot of include/q2048.h): where a key's row lies, how far a probe
// goes, what a row and a row-cache record are.  The HIP library and the CPU twin both compile THIS definition --
// that is what makes a host table a device table byte for byte -- and tests/test_core_host.py holds it against
// tests/table_model.py.  (The keys themselves, Geo<N>::Key, are in q2048_core5.hpp: the 5x5 one needs Board5.)
// ------------------------------------------------------------------------------------------
// Probe limits: beyond them a lookup reads "absent" and an update drops (counted; status TABLE_FULL).  They are
// what makes a probe of a FULL table end, not a load policy: at load 0.93 the longest cluster of a 2^22-slot
// table is already thousands of slots (ln n / (a - 1 - ln a)), and round 3's limit of 256 made "full" mean
// "load ~0.85" (a racing import at load 0.93 dropped rows).  Bulk moves of rows (import, the rehash of a growth)
// and q2048_q_lookup take kMaxProbe = 2^14 slots: they must place and find every row of a table the caller sized.
// The learning paths (rollouts, choose, update) take kRolloutProbe = 2^10: a lane of a rollout probes twice per
// step, and on a fixed table that has filled up 2^14 dependent 16-byte loads per probe made a launch orders of
// magnitude slower before TABLE_FULL became visible; 2^10 bounds that at ~load 0.93, where an
// absent key's expected probe is 100 slots already.  (Or the whole table if smaller.)
constexpr uint32_t kMaxProbe = 1u << 14, kRolloutProbe = 1u << 10;
constexpr int kMaxCas = 16;      // TD compare-and-swap attempts before the update is simply stored
Q_HD uint32_t probe_limit(uint64_t mask, uint32_t maxp) {
  return mask >= (uint64_t)maxp ? maxp : (uint32_t)mask + 1u;
}
// what a probe returns instead of a slot index (>= 0): ~h (< 0), h = the empty slot that ended it -- the place an
// insert of the key would claim -- or kNoSlot when the probe limit was hit
constexpr int64_t kNoSlot = INT64_MIN;

// Probe sequence of a key: BUCKETISED.  A miss moves the whole 128-byte line (4 slots) the probed
// slot lies in, and what a lookup costs is the number of lines it touches, so a
// collision is resolved inside the line already fetched: the sequence starts at the home slot
// (hash & mask), visits the other three slots of that line cyclically -- L2 hits -- and only then
// moves on to the next line, same order.  Plain linear probing left the line at the first collision
// of every key whose home is a line's last slot.  (Slots are 32 B; with a 128-byte aligned table
// a group of four is exactly one line.  Any 16-byte aligned table works.)
struct Seq { uint64_t line0, lmask; uint32_t off; };
Q_HD Seq seq_of(uint64_t hash, uint64_t mask) {
  return Seq{(hash & mask) >> 2, mask >> 2, (uint32_t)hash & 3u};
}
Q_HD uint64_t seq_slot(const Seq& s, uint32_t p) {   // p-th slot of the sequence
  return (((s.line0 + (uint64_t)(p >> 2)) & s.lmask) << 2) | (uint64_t)((s.off + p) & 3u);
}
Q_HD uint32_t seq_pos(const Seq& s, uint64_t slot) { // inverse, for a slot on the sequence
  return ((uint32_t)(((slot >> 2) - s.line0) & s.lmask) << 2) | (((uint32_t)slot - s.off) & 3u);
}

struct Row { float q0, q1, q2, q3; };
Q_HD float row_get(const Row& r, int a) {
  return a == 0 ? r.q0 : a == 1 ? r.q1 : a == 2 ? r.q2 : r.q3;
}
Q_HD void row_set(Row& r, int a, float v) {          // (selects, not an address: a carried row stays in registers)
  r.q0 = a == 0 ? v : r.q0; r.q1 = a == 1 ? v : r.q1;
  r.q2 = a == 2 ? v : r.q2; r.q3 = a == 3 ? v : r.q3;
}
// a row stored in the canonical frame, read in the frame of the env whose board has the canonical image g:
// Q_env[a] = Q_canon[pi_g(a)] (Q2048_FLAG_SYMMETRIC).  (static: g++ keeps it out of line in places, and there it
// stays a local symbol of the CPU twin, as it was)
static Q_HD Row row_env(const Row& r, uint32_t g) {
  return Row{row_get(r, sym_action(g, 0)), row_get(r, sym_action(g, 1)), row_get(r, sym_action(g, 2)),
             row_get(r, sym_action(g, 3))};
}

// Row cache of the 4-call API (optional, caller-owned, one record per env): what the fused rollout
// carries in registers from one step to the next -- the row this env read as s' in its last
// update, with its slot -- handed from one q_update call to the next q_choose / q_update through
// HBM as a coalesced stream.  s of step t + 1 is s' of step t unless an episode began, so the
// update then needs ONE scattered row read (s') instead of two, and a greedy choose none.  A
// record is used only when its key equals the key of the board actually passed in (0 = empty), so
// any calling pattern is correct; like the register-carried row it does not see what OTHER envs
// wrote to that row since.
template <int N> struct RowCache;
template <> struct RowCache<4> { uint64_t key; float q[4]; uint64_t slot; };                                // 32 B
template <> struct RowCache<5> { uint64_t key; float q[4]; uint64_t key_hi; uint64_t slot; uint64_t pad; }; // 48 B
static_assert(sizeof(RowCache<4>) == 32 && sizeof(RowCache<5>) == 48, "ABI layout");

// A record also carries, in the 24 bits above its 40-bit slot index, a TAG of the table it was read from (a hash
// of the table's address and capacity): a record left by a launch on another table -- the table has grown, or the
// caller switched tables and did not zero the cache -- never matches, so its slot index is never used against the
// wrong table (records outlive launches since round 4 and were trusted on a key match alone).  A table
// rewritten IN PLACE (zero-filled, imported into) keeps its tag: the caller zero-fills the cache then, as before.
Q_HD uint64_t cache_tag(const void* table, uint64_t mask) {
  return (mix64((uint64_t)reinterpret_cast<uintptr_t>(table) ^ (mask * 0x9E3779B97F4A7C15ull)) >> 40) << 40;
}
constexpr uint64_t kCacheSlotMask = (1ull << 40) - 1ull;
// VISIT ROWS (Q2048_FLAG_NO_NEW_ROWS).  With the key set closed a state without a row reads as the zero row the
// defaultdict would have created -- and while the env STAYS in that state (invalid moves) that fresh row learns as the
// defaultdict's would (Agent/main.py:43): the lane keeps it in the registers that otherwise carry the table's row, so
// that the first invalid move's negative reward sends argmax on to the next action instead of repeating action 0 until
// the stall rule ends the episode.  It is never part of the table and ends when the env leaves the state.  Across a
// launch boundary it travels like any carried row, through the row cache, as a ROWLESS record: slot field all ones
// (no table of 2^40 slots exists).  Only calls that carry the flag write or accept such records.
constexpr uint64_t kCacheRowless = kCacheSlotMask;

// ------------------------------------------------------------------------------------------
// LINE SUMMARIES of a table whose key set is closed (include/q2048.h, Q2048_FLAG_LINE_SUMMARY): one 64-bit
// word per 128-byte line of four slots, bits 16r..16r+15 = 0 when slot r is empty, else the fingerprint of
// its key (bits 48..63 of the key's hash, | 1: never 0).  4x4 tables keep the word in the slots' spare
// field, 5x5 tables in an array beside the table (q2048_table_summarise_side).
// summary_decode turns a word into the slots a lookup still has to look at, in the order of the key's
// probe sequence (which enters the line at slot `off`): bit j of `ev` = the slot at position j, slot
// (off + j) & 3, is empty or carries the key's fingerprint; bit r of `empty` = slot r is empty.
// summary_pop takes them one by one: `absent` = the sequence ends at slot r (the key has no row),
// otherwise slot r is a candidate whose key words settle it.  The 5x5 kernels and the CPU twin both
// decide their closed-key-set lookups through these two functions.
// ------------------------------------------------------------------------------------------
Q_HD uint64_t summary_fp(uint64_t hash) { return ((hash >> 48) & 0xffffull) | 1ull; }   // never 0
struct SummaryHits { uint32_t ev, empty; };
Q_HD SummaryHits summary_decode(uint64_t word, uint64_t fp, uint32_t off) {
  uint32_t e = 0u, m = 0u;
#pragma unroll
  for (uint32_t r = 0; r < 4u; ++r) {
    const uint64_t f = (word >> (16u * r)) & 0xffffull;
    e |= (uint32_t)(f == 0ull) << r;
    m |= (uint32_t)(f == fp) << r;
  }
  return SummaryHits{(((e | m) | ((e | m) << 4)) >> (off & 3u)) & 15u, e};
}
Q_HD bool summary_pop(SummaryHits& h, uint32_t off, uint32_t& r, bool& absent) {
  if (h.ev == 0u) return false;
  r = (off + (uint32_t)__builtin_ctz(h.ev)) & 3u;
  absent = ((h.empty >> r) & 1u) != 0u;
  h.ev &= h.ev - 1u;
  return true;
}

// np.argmax: first maximum (Agent/main.py:38,41)
Q_HD int argmax4(float q0, float q1, float q2, float q3) {
  int b = 0;
  float m = q0;
  if (q1 > m) { m = q1; b = 1; }
  if (q2 > m) { m = q2; b = 2; }
  if (q3 > m) { m = q3; b = 3; }
  return b;
}
Q_HD float max4(float q0, float q1, float q2, float q3) { return fmaxf(fmaxf(q0, q1), fmaxf(q2, q3)); }

// choose_action (Agent/main.py:34-38)
Q_HD int eps_greedy(double eps, uint32_t x_eps, uint32_t x_act, float q0, float q1, float q2,
                    float q3, bool& explored) {
  explored = draw_uniform(x_eps) < eps;                       // :35
  return explored ? draw_action(x_act) : argmax4(q0, q1, q2, q3);  // :36 / :38
}

// The same test on integers.  draw_uniform(x) = x * 2^-32 is exact in a double, and so is eps * 2^32 (a change
// of exponent), hence x * 2^-32 < eps <=> x < eps * 2^32 <=> x < ceil(eps * 2^32) for the integer x.
// eps_threshold is that bound, clamped to [0, 2^32] (eps <= 0 or NaN: never; eps >= 1: always) -- computed
// once per launch, the step compares one integer instead of cvt + mul + cmp in f64.
Q_HD uint64_t eps_threshold(double eps) {
  if (!(eps > 0.0)) return 0ull;
  if (eps >= 1.0) return 1ull << 32;
  return (uint64_t)ceil(eps * 4294967296.0);
}
Q_HD bool draw_below(uint32_t x, uint64_t threshold) {
  return (threshold >> 32) != 0ull || x < (uint32_t)threshold;
}
Q_HD int eps_greedy_at(uint64_t threshold, uint32_t x_eps, uint32_t x_act, float q0, float q1, float q2,
                       float q3, bool& explored) {
  explored = draw_below(x_eps, threshold);                    // :35
  return explored ? draw_action(x_act) : argmax4(q0, q1, q2, q3);  // :36 / :38
}

// ------------------------------------------------------------------------------------------
// the greedy PLAYER's decision (q2048_play_rollout; kernel and CPU twin both decide through these two)
// ------------------------------------------------------------------------------------------
// legal-move mask: bit a is set iff action a would change the board -- the trial-move loop of
// Deep_QLearning/main_dir/mainDQL_CNN_step2.py:168-174 (`env.game.move(action, trial=True)`), what
// q2048_legal_moves writes.  Four trial moves on a copy; only the four answers are kept.
template <class BoardT>
Q_HD uint32_t legal_mask(const BoardT& b) {
  uint32_t m = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    BoardT t = b;
    uint32_t score;
    m |= (uint32_t)move(t, a, score) << a;
  }
  return m;
}
// The move of a player that only makes moves that change the board.  Greedy: the first maximum of the row over
// the legal moves, ascending action order, strict > (np.argmax of the masked row, Agent/main.py:34-38 restricted
// to the mask; +0 and -0 compare equal).  Exploring (x_eps below the launch's eps_threshold): the k-th legal move
// in ascending order, k = (x_act * n_legal) >> 32.  No legal move: action 0, never counted as explored.
Q_HD int play_action(uint32_t legal, float q0, float q1, float q2, float q3, uint64_t threshold, uint32_t x_eps,
                     uint32_t x_act, bool& explored) {
  legal &= 15u;
  const uint32_t n_legal = popc(legal);
  explored = n_legal != 0u && draw_below(x_eps, threshold);
  if (explored) {
    uint32_t k = draw_index(x_act, n_legal), m = legal;
#pragma unroll
    for (int j = 0; j < 3; ++j) { const bool drop = k != 0u; m &= drop ? m - 1u : m; k -= drop ? 1u : 0u; }
    return __builtin_ctz(m);
  }
  int best = 0;
  float top = 0.f;
  bool have = false;
  if (legal & 1u) { top = q0; have = true; }
  if ((legal & 2u) && (!have || q1 > top)) { top = q1; best = 1; have = true; }
  if ((legal & 4u) && (!have || q2 > top)) { top = q2; best = 2; have = true; }
  if ((legal & 8u) && (!have || q3 > top)) { top = q3; best = 3; }
  return best;
}

// update_q_value (Agent/main.py:41-43) in the reference's own double arithmetic: no fused
// multiply-add (CPython rounds the product and the sum separately, and so does the oracle), so the
// device's doubles equal the oracle's bit for bit and only the final float32 store differs from the
// reference's float64 dict.
#if defined(__clang__)
#define Q2048_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define Q2048_NO_CONTRACT
#endif
Q_HD double td_target(float reward, float max_q_next, bool done, double gamma) {
  Q2048_NO_CONTRACT
  const double bootstrap = gamma * (double)max_q_next;
  return (double)reward + bootstrap * (done ? 0.0 : 1.0);                                     // :42
}
Q_HD double td_fold(double q, double target, double lr) {
  Q2048_NO_CONTRACT
  const double step = lr * (target - q);
  return q + step;                                                                            // :43
}
// returns the new Q[s][a] given the current one
Q_HD float td_value(float q_sa, float reward, float max_q_next, bool done, double lr,
                    double gamma) {
  return (float)td_fold((double)q_sa, td_target(reward, max_q_next, done, gamma), lr);
}

// ------------------------------------------------------------------------------------------
// FOLDING A PLAIN TABLE INTO A SYMMETRY-FOLDED ONE (include/q2048.h, q2048_table_fold; kernel and CPU twin both
// walk an orbit through fold_orbit).  The rows of the up to eight mirror images of a board become the one row of
// their canonical image.  The MEMBERS of the orbit of the canonical key c are image_h(c), h = 0..7 in ascending
// h, an h whose key equals that of a smaller h left out (boards with a stabiliser); the PRESENT members are the
// ones with a row in the source.  A member's row enters the canonical frame by its own g (the smallest g with
// image_g(member) = c, what the fused rollout uses when it meets that board): Qc[pi_g(a)] = Q_member[a].  The
// present members' rows are combined per action in member order, float32, every sum and product rounded on its
// own, the division a multiplication by float32(1.0 / k).
// ------------------------------------------------------------------------------------------
constexpr int kFoldMean = 0, kFoldMeanTrained = 1, kFoldSum = 2, kFoldMaxAbs = 3;   // Q2048_FOLD_*
// image_h(k), h = 0..7 (the candidates of canonical_key, in its order)
Q_HD void key_images(uint64_t k, uint64_t img[8]) {
  const uint64_t t = key_transpose(k), hk = key_flip_h(k), ht = key_flip_h(t);
  img[0] = k; img[1] = key_flip_v(t); img[2] = key_flip_v(hk); img[3] = ht;
  img[4] = hk; img[5] = t; img[6] = key_flip_v(k); img[7] = key_flip_v(ht);
}
Q_HD float fold_inv(uint32_t k) {               // float32(1.0 / k), k = 1..8: the mean is a product, never a `/`
  return k == 1u ? 1.0f : k == 2u ? 0.5f : k == 3u ? (float)(1.0 / 3.0) : k == 4u ? 0.25f : k == 5u ? (float)(1.0 / 5.0)
       : k == 6u ? (float)(1.0 / 6.0) : k == 7u ? (float)(1.0 / 7.0) : 0.125f;
}
// the entry x of the next member joins its action's running value (`n` entries have joined before; the first one
// is taken as it is -- no 0 + x, so a lone -0.0 stays -0.0)
template <int FOLD>
Q_HD void fold_step(float& acc, uint32_t& n, float x) {
  Q2048_NO_CONTRACT
  if (FOLD == kFoldMeanTrained && x == 0.0f) return;      // an untrained entry (+0 or -0) does not dilute a trained one
  if (n == 0u) acc = x;
  else if (FOLD == kFoldMaxAbs) acc = fabsf(x) > fabsf(acc) ? x : acc;   // equal magnitude: the earlier member's
  else acc = acc + x;
  n += 1u;
}
template <int FOLD>
Q_HD float fold_finish(float acc, uint32_t n) {
  Q2048_NO_CONTRACT
  if (FOLD == kFoldMean || FOLD == kFoldMeanTrained) {
    const float inv = fold_inv(n);
    return n == 0u ? 0.0f : acc * inv;                    // (MEAN_TRAINED with no trained entry: +0.0)
  }
  return acc;
}
// The orbit of the source row (m, q[4]), seen from that row.  `find(key, out[4])` says whether `key` has a row in
// the source and reads it.  Returns false when a present member precedes m: m is not its orbit's LEADER and
// another row's call returns true for this orbit.  For the leader: true, `canon` = the canonical key, r[4] = the
// orbit's row.  Exactly one present member of every orbit is its leader, so a caller that writes only for leaders
// writes every destination row once.
template <int FOLD, class Find>
Q_HD bool fold_orbit(uint64_t m, const float q[4], const Find& find, uint64_t& canon, float r[4]) {
  canon = canonical_key(m).key;
  uint64_t img[8];
  key_images(canon, img);
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t n[4] = {0u, 0u, 0u, 0u};
  bool leader = false;
#pragma unroll
  for (int h = 0; h < 8; ++h) {
    bool repeat = false;
#pragma unroll
    for (int j = 0; j < h; ++j) repeat |= img[j] == img[h];
    if (repeat) continue;
    float v[4];
    if (img[h] == m) {
      leader = true;
      v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
      if (!find(img[h], v)) continue;
      if (!leader) return false;
    }
    const uint32_t g = canonical_key(img[h]).g;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int at = sym_action(g, a);
#pragma unroll
      for (int b = 0; b < 4; ++b)               // (selects, not an index: the accumulators stay in registers)
        if (at == b) fold_step<FOLD>(acc[b], n[b], v[a]);
    }
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) r[b] = fold_finish<FOLD>(acc[b], n[b]);
  return true;
}

// ------------------------------------------------------------------------------------------
// UNFOLDING A SYMMETRY-FOLDED TABLE INTO A PLAIN ONE (include/q2048.h, q2048_table_unfold; kernel and CPU twin both
// walk an orbit through unfold_orbit): the fold's inverse.  The source row (c, Qc) -- c a canonical key, Qc in the
// canonical frame -- becomes one row per MEMBER of c's orbit (the fold's members, in its order), each in the
// member's own frame: Q_m[a] = Qc[pi_g(a)], g = canonical_key(m).g, what the fused rollout reads when it meets m.
// ------------------------------------------------------------------------------------------
// image_h(k) for one h (key_images computes all eight; this one is for a loop that is not unrolled)
Q_HD uint64_t key_image(uint64_t k, uint32_t h) {
  uint64_t o = (h & 1u) ? key_transpose(k) : k;                      // h odd: the images of T b
  o = ((0x9cu >> h) & 1u) ? key_flip_h(o) : o;                       // H for h in {2, 3, 4, 7}
  return ((0xc6u >> h) & 1u) ? key_flip_v(o) : o;                    // V for h in {1, 2, 6, 7}
}
// Calls emit(member key, member row) for every member of the orbit of `c`, in ascending h, and returns how many
// there are (8, 4, 2 or 1); returns 0 and emits nothing when `c` is not a canonical key (such a row has no place
// in a folded table: its orbit belongs to the row of canonical_key(c).key).  Distinct canonical keys have
// disjoint orbits, so a caller that gives every source row to one thread has one writer per destination row.
// The member loop is a loop, not eight copies of `emit`: a member costs a find-or-create in memory, and beside
// that the arithmetic of recomputing its key and its g (canonical_key(m).g itself -- no table of inverses to
// keep true for boards with a stabiliser) is free.
template <class Emit>
Q_HD uint32_t unfold_orbit(uint64_t c, const Row& qc, const Emit& emit) {
  uint64_t img[8];
  key_images(c, img);
  uint32_t first = 1u;                           // bit h: image h is not the image of a smaller h
#pragma unroll
  for (int h = 1; h < 8; ++h) {
    if (img[h] < c) return 0u;                   // (canonical_key(c).key != c)
    bool repeat = false;
#pragma unroll
    for (int j = 0; j < h; ++j) repeat |= img[j] == img[h];
    first |= (repeat ? 0u : 1u) << h;
  }
#pragma unroll 1
  for (uint32_t h = 0; h < 8u; ++h) {            // (h = 0: c itself, g = 0, the row as it is)
    if (!((first >> h) & 1u)) continue;
    const uint64_t m = key_image(c, h);
    emit(m, row_env(qc, canonical_key(m).g));
  }
  return popc(first);
}

// ------------------------------------------------------------------------------------------
// row-tuple linear Q (BASELINE configs[1]: "flat-array Q over row-tuple features").  NOT the
// reference's learner (its Q is keyed by the whole board, Agent/main.py:82): Q(s,a) is the sum
// over the four rows r of W[r][idx_r(s)][a] with idx_r = pack_row(row r); same epsilon-greedy
// and TD target as Agent/main.py:34-43, the error spread evenly over the four weights.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kRtIdx = 65536u;  // entries per row table; W is float[4][65536][4]
Q_HD float rt_sum(float e0, float e1, float e2, float e3) { return (e0 + e1) + (e2 + e3); }
Q_HD float rt_delta(float q_sa, float reward, float max_next, bool done, double lr, double gamma) {
  const double target = (double)reward + (gamma * (double)max_next * (done ? 0.0 : 1.0));
  return (float)((lr * 0.25) * (target - (double)q_sa));
}

// line-tuple linear Q: the four rows and the four columns as features ("all lines"), W = float[8][65536][4].
// Feature f < 4 is row f (the row-tuple index), feature 4 + c is pack_row of word c of transpose(b).  Q is the
// row-tuple sum of the rows plus the same sum of the columns; the error is spread evenly over the eight weights.
constexpr int kLtFeatures = 8;
Q_HD float lt_sum(float e0, float e1, float e2, float e3, float e4, float e5, float e6, float e7) {
  return rt_sum(e0, e1, e2, e3) + rt_sum(e4, e5, e6, e7);
}
Q_HD float lt_delta(float q_sa, float reward, float max_next, bool done, double lr, double gamma) {
  const double target = (double)reward + (gamma * (double)max_next * (done ? 0.0 : 1.0));
  return (float)((lr * 0.125) * (target - (double)q_sa));
}
// the eight indices of a board: ONE transpose per state serves the four column features
struct LtIdx { uint32_t i[kLtFeatures]; };
Q_HD LtIdx lt_indices(const Board& b) {
  const Board t = transpose(b);
  return LtIdx{{pack_row(b.r0), pack_row(b.r1), pack_row(b.r2), pack_row(b.r3),
                pack_row(t.r0), pack_row(t.r1), pack_row(t.r2), pack_row(t.r3)}};
}

// ------------------------------------------------------------------------------------------
// afterstate value learner on the line features: V = float[8][65536], one value per line entry, indexed by
// lt_indices.  A state is judged by the four boards its moves lead to BEFORE the spawn (the afterstates):
//   c_a = s moved by a (move(), its score and its "changed" flag), q_a = (float)score_a + v(c_a),
//   v(x) = lt_sum of the eight entries of x.
// The choice is the player's (play_action over the moves that change the board), the TD step moves v(c_a) of the
// move played towards gamma * best(s'), best(s') = q at the greedy legal move of the next state (0 if it has none).
// ------------------------------------------------------------------------------------------
// move() that also hands out the transpose of the moved board: both exist inside it (the slide works on "cell j of
// every line" words, which are the board for a vertical move and its transpose for a horizontal one), so the eight
// indices of an afterstate need no transpose of their own.  Same answers as move(), bit for bit.
Q_HD bool move_with_transpose(Board& b, Board& bt, int action, uint32_t& score) {
  const bool horiz = (action & 1) == 0;
  const bool rev = (action & 2) != 0;
  const Board t = transpose(b);
  const uint32_t p0 = horiz ? t.r0 : b.r0, p1 = horiz ? t.r1 : b.r1;
  const uint32_t p2 = horiz ? t.r2 : b.r2, p3 = horiz ? t.r3 : b.r3;
  uint32_t c0 = rev ? p3 : p0, c1 = rev ? p2 : p1, c2 = rev ? p1 : p2, c3 = rev ? p0 : p3;
  const uint32_t o0 = c0, o1 = c1, o2 = c2, o3 = c3;
  score = slide_lines(c0, c1, c2, c3);
  const bool moved = ((c0 ^ o0) | (c1 ^ o1) | (c2 ^ o2) | (c3 ^ o3)) != 0;
  const Board q{rev ? c3 : c0, rev ? c2 : c1, rev ? c1 : c2, rev ? c0 : c3};
  const Board qt = transpose(q);
  b = horiz ? qt : q;
  bt = horiz ? q : qt;
  return moved;
}
// the eight indices of a board whose transpose is at hand
Q_HD LtIdx lt_indices_of(const Board& b, const Board& t) {
  return LtIdx{{pack_row(b.r0), pack_row(b.r1), pack_row(b.r2), pack_row(b.r3),
                pack_row(t.r0), pack_row(t.r1), pack_row(t.r2), pack_row(t.r3)}};
}
// the four candidates of a state: indices of c_a, merge score, and the mask of the moves that change the board
struct AvCands { LtIdx x[4]; uint32_t score[4]; uint32_t legal; };
Q_HD AvCands av_candidates(const Board& s) {
  AvCands c;
  c.legal = 0u;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    Board m = s, mt;
    c.legal |= (uint32_t)move_with_transpose(m, mt, a, c.score[a]) << a;
    c.x[a] = lt_indices_of(m, mt);
  }
  return c;
}
Q_HD float av_v(const float e[kLtFeatures]) { return lt_sum(e[0], e[1], e[2], e[3], e[4], e[5], e[6], e[7]); }
Q_HD float av_q(uint32_t score, float v) { return (float)score + v; }
// best(s): q at the action play_action picks with threshold 0 (first maximum over the legal moves, strict >);
// 0 without a legal move
Q_HD float av_best(uint32_t legal, const Row& q) {
  bool explored;
  const int a = play_action(legal, q.q0, q.q1, q.q2, q.q3, 0ull, 0u, 0u, explored);
  return (legal & 15u) ? row_get(q, a) : 0.0f;
}
// One evaluation of a state: the candidates and their 32 gathered entries (each library gathers in its own way).
struct AvEval { AvCands c; float e[4][kLtFeatures]; };
Q_HD Row av_row(const AvEval& ev) {
  return Row{av_q(ev.c.score[0], av_v(ev.e[0])), av_q(ev.c.score[1], av_v(ev.e[1])),
             av_q(ev.c.score[2], av_v(ev.e[2])), av_q(ev.c.score[3], av_v(ev.e[3]))};
}
// the afterstate of the move played, out of an evaluation: its indices and the entries gathered for it (selects,
// not an address: an evaluation stays in registers)
struct AvTaken { LtIdx x; float e[kLtFeatures]; };
// (the four values are passed BY VALUE: all four are read, then selected.  A ternary over the array elements
// themselves becomes one load at an address computed from `a`, and the evaluation then lives in scratch memory.
// Two bit tests, a = 0..3: a chain of a == k becomes a switch, which hipcc lowers to a tree of branches per value.)
Q_HD uint32_t av_sel(int a, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
  const uint32_t lo = (a & 1) ? v1 : v0, hi = (a & 1) ? v3 : v2;
  return (a & 2) ? hi : lo;
}
Q_HD float av_sel(int a, float v0, float v1, float v2, float v3) {
  const float lo = (a & 1) ? v1 : v0, hi = (a & 1) ? v3 : v2;
  return (a & 2) ? hi : lo;
}
Q_HD AvTaken av_taken(const AvEval& ev, int act) {
  AvTaken t;
#pragma unroll
  for (int f = 0; f < kLtFeatures; ++f) {
    t.x.i[f] = av_sel(act, ev.c.x[0].i[f], ev.c.x[1].i[f], ev.c.x[2].i[f], ev.c.x[3].i[f]);
    t.e[f] = av_sel(act, ev.e[0][f], ev.e[1][f], ev.e[2][f], ev.e[3][f]);
  }
  return t;
}
// THE CARRIED-ENTRY RULE of the fused learner: `ev` was gathered before the TD write of `t` (+ d), so every entry
// of it at a written (feature, index) takes the written value.
Q_HD void av_carry(AvEval& ev, const AvTaken& t, float d) {
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int f = 0; f < kLtFeatures; ++f)
      if (ev.c.x[a].i[f] == t.x.i[f]) ev.e[a][f] = t.e[f] + d;
}
// d of the TD step: `live` = the next state is not terminal (not done, and it has a move)
Q_HD float av_delta(float v_x, float best_next, bool live, double lr, double gamma) {
  Q2048_NO_CONTRACT
  const double target = (gamma * (double)best_next) * (live ? 1.0 : 0.0);
  return (float)((lr * 0.125) * (target - (double)v_x));
}

// ------------------------------------------------------------------------------------------
// 6-tuple afterstate network with shared symmetric weights (q2048_nt_*): V = float[4][2^24], 256 MiB.  Four 6-cell
// patterns (cell index 4r + c), each read on the eight images of the board (key_images: the numbering of
// Q2048_FLAG_SYMMETRIC), one table per pattern shared by the eight images:
//   P0 = {0,1,2,3,4,5}   P1 = {4,5,6,7,8,9}   P2 = {0,1,2,4,5,6}   P3 = {4,5,6,8,9,10}
//   idx[p][g](x) = sum_k (img_g(x).flat[P_p[k]] & 15) << 4k;  e[p][g] = V[p][idx[p][g](x)];
//   v(x) = rt_sum(s_0, s_1, s_2, s_3), s_p = lt_sum(e[p][0..7]).
// Everything else -- candidates, q_a, best, the choice, live and target of the TD step -- is the afterstate
// family's, by calling it.  The two libraries hand in how an entry is loaded and stored (`ld(p, idx)`,
// `st(p, idx, value)`); what is loaded, in which order it is summed and what is stored is written here once.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kNtIdx = 1u << 24;   // entries per pattern table
constexpr int kNtPatterns = 4, kNtImages = 8;
// The four indices of an image from its packed key (cell 4r + c in nibble 4r + c): P0 is the low six nibbles, P1
// the same one row down, P2 three nibbles of row 0 and three of row 1, P3 the same one row down.
Q_HD uint32_t nt_index(uint64_t key, int p) {
  const uint32_t k = (uint32_t)((p & 1) ? (key >> 16) : key), k1 = (uint32_t)(key >> ((p & 1) ? 32 : 16));
  return (p & 2) ? ((k & 0xfffu) | ((k1 & 0xfffu) << 12)) : (k & 0xffffffu);
}
struct NtIdx { uint32_t i[kNtPatterns][kNtImages]; };
// the 32 indices of a board from its packed key: all an evaluation or an update needs of the board
Q_HD NtIdx nt_indices_key(uint64_t key) {
  uint64_t img[kNtImages];
  key_images(key, img);
  NtIdx ix;
#pragma unroll
  for (int p = 0; p < kNtPatterns; ++p)
#pragma unroll
    for (int g = 0; g < kNtImages; ++g) ix.i[p][g] = nt_index(img[g], p);
  return ix;
}
Q_HD NtIdx nt_indices(const Board& x) {
  bool overflow;                                  // a cell >= 16 aliases by its low nibble, as in the other families
  return nt_indices_key(pack_key(x, overflow));
}
struct NtEntries { float e[kNtPatterns][kNtImages]; };
// all 32 entries of a board, loaded back to back: nothing between two loads but the next address
template <class Ld>
Q_HD NtEntries nt_gather(const NtIdx& ix, Ld ld) {
  NtEntries n;
#pragma unroll
  for (int p = 0; p < kNtPatterns; ++p)
#pragma unroll
    for (int g = 0; g < kNtImages; ++g) n.e[p][g] = ld(p, ix.i[p][g]);
  return n;
}
Q_HD float nt_v(const NtEntries& n) {
  float s[kNtPatterns];
#pragma unroll
  for (int p = 0; p < kNtPatterns; ++p)
    s[p] = lt_sum(n.e[p][0], n.e[p][1], n.e[p][2], n.e[p][3], n.e[p][4], n.e[p][5], n.e[p][6], n.e[p][7]);
  return rt_sum(s[0], s[1], s[2], s[3]);
}
// One evaluation of a state: each candidate's 32 entries are reduced to its q as they arrive, so what is held is a
// Row and the mask of the moves that change the board -- nothing is carried from step to step.  The four candidates
// are a LOOP, not four copies: unrolled, hipcc keeps the 128 entries of an evaluation and their addresses alive
// together (it sinks the sums below the last load), which takes every VGPR there is and spills; as a loop a lane has
// 32 loads in flight, the other waves of the SIMD fill the wait, and the code is a quarter as long.  (The selects:
// an array indexed by the loop counter would live in scratch memory.)
struct NtEval { Row q; uint32_t legal; };
template <class Ld>
Q_HD NtEval nt_eval(const Board& s, Ld ld) {
  NtEval ev{Row{0.0f, 0.0f, 0.0f, 0.0f}, 0u};
#pragma unroll 1
  for (int a = 0; a < 4; ++a) {
    Board m = s;
    uint32_t score;
    ev.legal |= (uint32_t)move(m, a, score) << a;
    const float q = av_q(score, nt_v(nt_gather(nt_indices(m), ld)));
    ev.q.q0 = a == 0 ? q : ev.q.q0;
    ev.q.q1 = a == 1 ? q : ev.q.q1;
    ev.q.q2 = a == 2 ? q : ev.q.q2;
    ev.q.q3 = a == 3 ? q : ev.q.q3;
  }
  return ev;
}
// d of the TD step: av_delta's live and target, the error spread over the 32 entries
Q_HD float nt_delta(float v_x, float best_next, bool live, double lr, double gamma) {
  Q2048_NO_CONTRACT
  const double target = (gamma * (double)best_next) * (live ? 1.0 : 0.0);
  return (float)((lr * 0.03125) * (target - (double)v_x));
}
// The TD step on the afterstate x, given the evaluation of the next state: all 32 entries of x are gathered, then
// each is written as gathered + d.  Entries of x that are the same weight (a board with a symmetry) gathered the
// same value and store the same value, so that weight moves by d ONCE: this family's rule, not the literature's.
template <class Ld, class St>
Q_HD void nt_td(const Board& x, const NtEval& en, bool done, double lr, double gamma, Ld ld, St st) {
  const NtIdx ix = nt_indices(x);
  const NtEntries n = nt_gather(ix, ld);
  const bool live = !done && en.legal != 0u;
  const float d = nt_delta(nt_v(n), av_best(en.legal, en.q), live, lr, gamma);
#pragma unroll
  for (int p = 0; p < kNtPatterns; ++p)
#pragma unroll
    for (int g = 0; g < kNtImages; ++g) st(p, ix.i[p][g], n.e[p][g] + d);
}

// TD(lambda) WITH A TRUNCATED TRACE (q2048_nt_lambda_*): a lane remembers the packed keys of the last n <= h <= 3
// afterstates it learned on in the current episode, newest first, and the error of a step also moves them:
//   d_0 = (float)((lr / 32) * err)            on the 32 entries of x     (nt_delta's d bit for bit: nt_td's write)
//   d_k = (float)(((lr / 32) * L_k) * err)    on the 32 entries of key k, k = 1..n;  L_1 = lambda, L_k = L_{k-1} * lambda
// in ASCENDING k, each gather after the stores before it: a weight that x and an earlier afterstate share moves by d_0
// and then by d_k (the definition is sequential; within one key a repeated weight moves once, the family's rule).
// No value is summed for k >= 1.  `cut` (the move was explored: Watkins' cut) empties the trace BEFORE the step,
// `done` after it.  In memory a trace is uint64_t[4] = {n, key_1, key_2, key_3}, every word beyond n zero.
struct NtTrace { uint64_t k1, k2, k3; uint32_t n; };
Q_HD void nt_trace_clear(NtTrace& tr) { tr.k1 = tr.k2 = tr.k3 = 0ull; tr.n = 0u; }
// h >= 1 (h == 0 is nt_td and no trace: the callers' branch)
template <class Ld, class St>
Q_HD void nt_lambda_td(const Board& x, const NtEval& en, bool done, bool cut, double lr, double gamma, double lambda,
                       uint32_t h, NtTrace& tr, Ld ld, St st) {
  Q2048_NO_CONTRACT
  if (cut) nt_trace_clear(tr);
  bool overflow;
  const uint64_t key = pack_key(x, overflow);
  double err;
  {
    const NtIdx ix = nt_indices_key(key);
    const NtEntries n = nt_gather(ix, ld);
    const bool live = !done && en.legal != 0u;
    const double target = (gamma * (double)av_best(en.legal, en.q)) * (live ? 1.0 : 0.0);   // nt_delta's
    err = target - (double)nt_v(n);
    const float d = (float)((lr * 0.03125) * err);
#pragma unroll
    for (int p = 0; p < kNtPatterns; ++p)
#pragma unroll
      for (int g = 0; g < kNtImages; ++g) st(p, ix.i[p][g], n.e[p][g] + d);
  }
  // The earlier afterstates are a LOOP (one copy of the 32 loads and 32 stores), and the key of turn k is always
  // `cur`: the others move up behind it.  An array indexed by k would live in scratch memory (see nt_eval).
  uint64_t cur = tr.k1, nx1 = tr.k2, nx2 = tr.k3;
  double L = lambda;
#pragma unroll 1
  for (uint32_t k = 0; k < tr.n; ++k) {
    const float d = (float)(((lr * 0.03125) * L) * err);
    const NtIdx ix = nt_indices_key(cur);
    const NtEntries n = nt_gather(ix, ld);
#pragma unroll
    for (int p = 0; p < kNtPatterns; ++p)
#pragma unroll
      for (int g = 0; g < kNtImages; ++g) st(p, ix.i[p][g], n.e[p][g] + d);
    cur = nx1;
    nx1 = nx2;
    L = L * lambda;
  }
  if (done) { nt_trace_clear(tr); return; }
  tr.k3 = h >= 3u ? tr.k2 : 0ull;
  tr.k2 = h >= 2u ? tr.k1 : 0ull;
  tr.k1 = key;
  tr.n = tr.n + 1u < h ? tr.n + 1u : h;
}
// the memory image of a trace
Q_HD void nt_trace_words(const NtTrace& tr, uint64_t w[4]) { w[0] = tr.n; w[1] = tr.k1; w[2] = tr.k2; w[3] = tr.k3; }
// (a trace from memory is taken as it is found -- a caller may hand in more keys than h, the next push truncates
// them -- but n, which decides how many keys are updated, is at most 3)
Q_HD NtTrace nt_trace_from(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
  return NtTrace{w1, w2, w3, w0 < 3u ? (uint32_t)w0 : 3u};
}

// THE STAGED NETWORK (q2048_nts_*): a table per stage of the game, V = float[S][4][2^24], 1 <= S <= 8.  The largest
// tile of a board selects its table.  `stages` holds the thresholds as nibbles: nibble i is t_{i+1}, a tile exponent
// in 1..15 (the tile 2^t); the thresholds ascend strictly, the nonzero nibbles are contiguous from nibble 0 and the
// top nibble is 0 (at most 7 thresholds); S = 1 + the number of nonzero nibbles; stages == 0 is the plain network.
//   maxnib(x) = the largest nibble of pack_key(x)   (a cell >= 16 aliases by its low nibble, exactly as in nt_index)
//   stage(x)  = the number of thresholds t_i with maxnib(x) >= t_i
//   v(x)      = nt_v over the 32 entries of x taken from table stage(x)
// In an evaluation of a state every candidate afterstate has its OWN stage: a merge that creates a threshold tile
// puts that candidate in the next table while its siblings stay below.  The TD step is nt_td on table stage(c_act);
// its target is the best of the staged evaluation of the next state.  q_a, best, the choice, live and target are the
// afterstate family's.  A stage only selects the base of the table: the libraries hand in `ld_of(stage)` /
// `st_of(stage)`, which give the `ld` / `st` of that table, and a staged evaluation makes the same 128 requests as a
// plain one.
constexpr int kNtsMaxStages = 8;
constexpr size_t kNtsStageFloats = (size_t)kNtPatterns * kNtIdx;   // floats per stage table
Q_HD bool nts_spec_ok(uint32_t stages) {
  uint32_t prev = 0u;
  bool ended = false;
  for (int i = 0; i < 8; ++i) {
    const uint32_t t = (stages >> (4 * i)) & 15u;
    if (t == 0u) { ended = true; continue; }
    if (ended || t <= prev || i == 7) return false;
    prev = t;
  }
  return true;
}
Q_HD uint32_t nts_count(uint32_t stages) {       // S of a well-formed spec
  uint32_t n = 1u;
  for (int i = 0; i < 7; ++i) n += ((stages >> (4 * i)) & 15u) != 0u;
  return n;
}
Q_HD uint32_t nts_maxnib(uint64_t key) {
  uint32_t m = 0u;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const uint32_t c = (uint32_t)(key >> (4 * i)) & 15u;
    m = c > m ? c : m;
  }
  return m;
}
// (seven compares and adds on a wave-uniform spec; a zero nibble counts for nothing)
Q_HD uint32_t nts_stage_of_key(uint64_t key, uint32_t stages) {
  const uint32_t m = nts_maxnib(key);
  uint32_t n = 0u;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const uint32_t t = (stages >> (4 * i)) & 15u;
    n += (uint32_t)(t != 0u && m >= t);
  }
  return n;
}
// the stage of a board, from the packed key that nt_indices forms too (one pack_key after inlining)
Q_HD uint32_t nts_stage(const Board& x, uint32_t stages) {
  bool overflow;
  return nts_stage_of_key(pack_key(x, overflow), stages);
}
template <class LdOf>
Q_HD float nts_v(const Board& x, uint32_t stages, LdOf ld_of) {
  return nt_v(nt_gather(nt_indices(x), ld_of(nts_stage(x, stages))));
}
// nt_eval with each candidate's entries from the table of its own stage
template <class LdOf>
Q_HD NtEval nts_eval(const Board& s, uint32_t stages, LdOf ld_of) {
  NtEval ev{Row{0.0f, 0.0f, 0.0f, 0.0f}, 0u};
#pragma unroll 1
  for (int a = 0; a < 4; ++a) {
    Board m = s;
    uint32_t score;
    ev.legal |= (uint32_t)move(m, a, score) << a;
    const float q = av_q(score, nts_v(m, stages, ld_of));
    ev.q.q0 = a == 0 ? q : ev.q.q0;
    ev.q.q1 = a == 1 ? q : ev.q.q1;
    ev.q.q2 = a == 2 ? q : ev.q.q2;
    ev.q.q3 = a == 3 ? q : ev.q.q3;
  }
  return ev;
}
// nt_td on the table of x's stage
template <class LdOf, class StOf>
Q_HD void nts_td(const Board& x, uint32_t stages, const NtEval& en, bool done, double lr, double gamma, LdOf ld_of,
                 StOf st_of) {
  const uint32_t k = nts_stage(x, stages);
  nt_td(x, en, done, lr, gamma, ld_of(k), st_of(k));
}
// PROMOTION (q2048_nts_promote), on every (p, idx): if the bit pattern of V[to][p][idx] is 0x00000000 and that of
// V[from][p][idx] is not, V[to][p][idx] takes the BITS of V[from][p][idx] (a NaN included); -0.0f counts as written.
Q_HD bool nts_promotes(uint32_t to_bits, uint32_t from_bits) { return to_bits == 0u && from_bits != 0u; }
// CAROUSEL SHAPING (q2048_car_*): training episodes start in turn at the beginning of every stage, from boards on
// which earlier games entered that stage.  Three buffers in the caller's memory:
//   pool   uint8 [S][P][32], 16-byte aligned: a ring of P >= 1 records per stage; row 0 is never read or written
//   counts uint64 [S]: counts[k] = records ever committed to stage k; n_k = min(counts[k], P) are valid, slots 0..n_k-1
//   fresh  uint8 [S][B][32], 16-byte aligned: one record per (stage, lane), written by the learner, consumed by the commit
// A RECORD is 32 bytes: the board (0..15), aux.score (16..19), the bits of aux.ep_return (20..23), zero (24..31).  A
// record whose 16 board bytes are zero is EMPTY; a board after a step holds a tile, so no real record is empty.
// RECORDING, in fused step t of lane i: k0 = nts_stage of the state the step starts from, k1 = that of the state
// env_step leaves (spawn included); if !done && k1 > k0, fresh[k1][i] takes the record of (b, a) as env_step left them.
// The last crossing of a lane into a stage within a launch wins, a jump over a stage records at k1 only, a restart
// records nothing.
// RESTART, in place of begin_episode: episode += 1, d = draws(seed, id, episode, kStreamReset), k = episode % S; k == 0
// or n_k == 0 is reset_board(b, a, d) -- begin_episode bit for bit -- otherwise the board, score and ep_return come from
// pool[k][(d.x0 * n_k) >> 32].  A restart writes what reset_board writes and nothing else of the lane.
// The pool and the counts are read-only during a launch and a lane writes only its own fresh[.][i]: at fixed weights
// a launch's boards, aux and records are a pure function of its inputs at any B.
// COMMIT, per stage k = 1..S-1: the lanes with a non-empty fresh[k][i] in ascending i, m of them, rank r among them;
// the record of rank r goes to pool[k][(counts[k] + r) % P] if r + P >= m (of more than P records the last P land,
// each in a slot of its own); then counts[k] += m and every consumed fresh[k][i] is zeroed whole.
constexpr int kCarRecordBytes = 32;
constexpr int64_t kCarMaxRing = (int64_t)1 << 32;      // P above this is Q2048_ERR_SIZE (the slot draw is 32 bits)
struct CarRecord { Board b; Words4 tail; };            // the two 16-byte halves of a record
static_assert(sizeof(CarRecord) == kCarRecordBytes, "a record is two 16-byte accesses");
Q_HD CarRecord car_record(const Board& b, const Aux& a) {
  return CarRecord{b, Words4{(uint32_t)a.score, f32_bits(a.ep_return), 0u, 0u}};
}
Q_HD bool car_empty(const Board& b) { return (b.r0 | b.r1 | b.r2 | b.r3) == 0u; }
Q_HD bool car_records(uint32_t k0, uint32_t k1, bool done) { return !done && k1 > k0; }
Q_HD uint64_t car_valid(uint64_t count, uint64_t P) { return count < P ? count : P; }
Q_HD uint32_t car_pick(uint32_t x0, uint64_t n) { return (uint32_t)(((uint64_t)x0 * n) >> 32); }
Q_HD bool car_lands(uint64_t r, uint64_t m, uint64_t P) { return r + P >= m; }
Q_HD uint64_t car_slot(uint64_t count, uint64_t r, uint64_t P) { return (count % P + r % P) % P; }   // (count + r) % P without the wrap at 2^64
// `valid(k)` gives n_k, `ld(k, j)` the record pool[k][j]; both are called in the restart-from-the-pool case only
template <class Valid, class LdRec>
Q_HD void car_restart(Board& b, Aux& a, uint64_t seed, uint64_t env_id, uint32_t S, Valid valid, LdRec ld) {
  a.episode += 1u;
  const Draws d = draws(seed, env_id, a.episode, kStreamReset);
  const uint32_t k = a.episode % S;
  const uint64_t n = k == 0u ? 0u : valid(k);
  if (n == 0u) {
    reset_board(b, a, d);
    return;
  }
  const CarRecord rec = ld(k, car_pick(d.x0, n));
  b = rec.b;
  a.score = (int32_t)rec.tail.w0;
  a.ep_return = bits_f32(rec.tail.w1);
}

// TEMPORAL-COHERENCE STEP SIZES for the network (q2048_nt_tc_*): beside V sits acc = float[4][2^24][2], acc[p][idx] =
// {E, A}: the signed sum of the TD errors that weight has seen and the sum of their magnitudes.  Its own rate is
// |E| / A: 1 while its errors agree in sign, towards 0 as they cancel.  A pair is loaded and stored whole (`ldp(p, idx)`,
// `stp(p, idx, pair)`: one 8-byte access each way in both libraries), so a stored pair derives from ONE earlier pair.
struct NtPair { float E, A; };
// the rate of a weight, in [0, 1] for ANY pair (a loaded file's included): no history, A <= 0 or a NaN give 1
// (the quotient is formed for every pair and selected afterwards: 32 divisions in straight-line code, no branch per entry)
Q_HD float nt_tc_rate(const NtPair& h) {
  const float r = fminf(fabsf(h.E) / h.A, 1.0f);
  return (h.A > 0.0f) ? r : 1.0f;
}
// err of the TD step, in double: nt_delta's live and target
Q_HD double nt_tc_err(float v_x, float best_next, bool live, double gamma) {
  Q2048_NO_CONTRACT
  const double target = (gamma * (double)best_next) * (live ? 1.0 : 0.0);
  return target - (double)v_x;
}
// d of one entry: nt_delta's product, times the entry's rate; at rate 1 it is nt_delta's d bit for bit
Q_HD float nt_tc_delta(double err, float rate, double lr) {
  Q2048_NO_CONTRACT
  return (float)(((lr * 0.03125) * err) * (double)rate);
}
// the pair after an error e: |E + e| <= A + |e| in exact arithmetic, and rounding to nearest is monotone and
// symmetric, so |E| <= A survives the two float32 additions exactly
Q_HD NtPair nt_tc_fold(const NtPair& h, float e) { return NtPair{h.E + e, h.A + fabsf(e)}; }
struct NtPairs { NtPair h[kNtPatterns][kNtImages]; };
// nt_index for a pattern number that is a loop counter: masks, not `?:` (on a uniform counter hipcc turns each `?:`
// into a branch)
Q_HD uint32_t nt_index_at(uint64_t key, uint32_t p) {
  const uint32_t sh = (p & 1u) << 4, split = 0u - ((p >> 1) & 1u);               // split: all ones for P2, P3
  const uint32_t k = (uint32_t)(key >> sh), k1 = (uint32_t)(key >> (sh + 16u));
  return (k & (0xffffffu ^ (split & 0xfff000u))) | (((k1 & 0xfffu) << 12) & split);
}
// nt_td with a rate per entry.  The 32 entries and the 32 pairs of x are gathered back to back (64 requests in
// flight together); then each entry is written as gathered + d_i and each pair as gathered + {e, |e|}.  Entries of x
// that are the same weight gathered the same value and the same pair and store the same, so that weight and its
// pair move ONCE: the family's rule.
template <class Ld, class LdP, class St, class StP>
Q_HD void nt_tc_td(const Board& x, const NtEval& en, bool done, double lr, double gamma, Ld ld, LdP ldp, St st,
                   StP stp) {
  bool overflow;
  uint64_t img[kNtImages];
  key_images(pack_key(x, overflow), img);
  NtEntries n;
  NtPairs h;
#pragma unroll
  for (int p = 0; p < kNtPatterns; ++p)
#pragma unroll
    for (int g = 0; g < kNtImages; ++g) n.e[p][g] = ld(p, nt_index(img[g], p));
#pragma unroll
  for (int p = 0; p < kNtPatterns; ++p)
#pragma unroll
    for (int g = 0; g < kNtImages; ++g) h.h[p][g] = ldp(p, nt_index(img[g], p));
  const bool live = !done && en.legal != 0u;
  const double err = nt_tc_err(nt_v(n), av_best(en.legal, en.q), live, gamma);
  const float e = (float)err;
  // The patterns are a LOOP, as the candidates of nt_eval are, and for its reason: what stays alive across it is the
  // eight image keys, the 32 values and the 32 pairs; the eight indices of a pattern are formed again from the keys
  // when they are stored to.  Unrolled, hipcc keeps the 32 load offsets of V, the 32 of acc and every quotient alive
  // beside them and needs more than 256 VGPRs.  The loop always works on row 0 and then moves the rows up by one: an
  // array indexed by the loop counter would live in scratch memory, and selects on the (uniform) counter become a
  // branch per entry.
#pragma unroll 1
  for (int p = 0; p < kNtPatterns; ++p) {
#pragma unroll
    for (int g = 0; g < kNtImages; ++g) {
      const uint32_t idx = nt_index_at(img[g], (uint32_t)p);
      st(p, idx, n.e[0][g] + nt_tc_delta(err, nt_tc_rate(h.h[0][g]), lr));
      stp(p, idx, nt_tc_fold(h.h[0][g], e));
    }
#pragma unroll
    for (int q = 0; q + 1 < kNtPatterns; ++q)
#pragma unroll
      for (int g = 0; g < kNtImages; ++g) {
        n.e[q][g] = n.e[q + 1][g];
        h.h[q][g] = h.h[q + 1][g];
      }
  }
}

// THE SYNCHRONOUS BATCH STEP (q2048_nt_sync_*): every lane evaluates against the same frozen V, the errors that fall
// on a weight are summed exactly, as integers, and the weight then moves once by their mean.  Beside V sits
// acc = uint64_t[4][2^24][2], acc[p][idx] = {S, C}: the two's-complement sum of the quantised errors and the number of
// contributions; all zero between steps.
//   phase A  a lane with a TD sample: err as nt_delta forms it, q = nt_sync_quantise(err), and for each of its 32
//            entries, PER OCCURRENCE, `add(p, idx, q)`: S += q, C += 1 (both atomic).  V is only read.
//   phase B  every weight with C != 0 is written exactly once: `claim(p, idx)` returns C and leaves 0 there, so of all
//            occurrences of a weight in the batch exactly one sees C != 0; its lane takes S (`take(p, idx)`: returns S,
//            leaves 0) and stores V + nt_sync_step(S, C, lr).
// The sums are integers (B <= 2^20: |S| <= 2^30 * 2^23 = 2^53, C <= 2^23, both exact in double), so the bytes do not
// depend on the order or the mechanism that forms them.  Between A and B every lane of A has finished: the callers'
// kernel boundary, or a join of the threads.
constexpr int64_t kNtSyncMaxB = (int64_t)1 << 20;
constexpr double kNtSyncClamp = 262144.0, kNtSyncScale = 4096.0;     // |err| <= 2^18 on a grid of 2^-12
// the clamp is exact, the product (by a power of two, below 2^31) is exact, llrint rounds to nearest even; a NaN is 0
Q_HD int64_t nt_sync_quantise(double err) {
  Q2048_NO_CONTRACT
  const double e = (err != err) ? 0.0 : err;
  const double c = e < -kNtSyncClamp ? -kNtSyncClamp : (e > kNtSyncClamp ? kNtSyncClamp : e);
  return (int64_t)llrint(c * kNtSyncScale);
}
// d of a weight from its sums: one division, one rounding to float32
Q_HD float nt_sync_step(int64_t S, uint64_t C, double lr) {
  Q2048_NO_CONTRACT
  const double m = (double)S / ((double)C * kNtSyncScale);
  return (float)((lr * 0.03125) * m);
}
// phase A on the afterstate x, given the evaluation of the next state; returns the packed key of x (never 0: an
// afterstate of a legal move is not the empty board), which is all phase B needs of the lane
template <class Ld, class Add>
Q_HD uint64_t nt_sync_acc(const Board& x, const NtEval& en, bool done, double gamma, Ld ld, Add add) {
  Q2048_NO_CONTRACT
  bool overflow;
  const uint64_t key = pack_key(x, overflow);
  const NtIdx ix = nt_indices_key(key);
  const NtEntries n = nt_gather(ix, ld);
  const bool live = !done && en.legal != 0u;
  const double target = (gamma * (double)av_best(en.legal, en.q)) * (live ? 1.0 : 0.0);   // nt_delta's
  const int64_t q = nt_sync_quantise(target - (double)nt_v(n));
#pragma unroll
  for (int p = 0; p < kNtPatterns; ++p)
#pragma unroll
    for (int g = 0; g < kNtImages; ++g) add(p, ix.i[p][g], q);
  return key;
}
// phase B of a lane that contributed `key`.  The patterns are a LOOP (see nt_tc_td): eight claims are in flight
// together, and V is loaded beside them whether the claim succeeds or not (a load of an entry nobody else writes
// before its one owner does, so the owner reads the frozen value).
template <class Ld, class St, class Claim, class Take>
Q_HD void nt_sync_apply(uint64_t key, double lr, Ld ld, St st, Claim claim, Take take) {
  uint64_t img[kNtImages];
  key_images(key, img);
#pragma unroll 1
  for (int p = 0; p < kNtPatterns; ++p) {
    uint64_t c[kNtImages];
    float v[kNtImages];
#pragma unroll
    for (int g = 0; g < kNtImages; ++g) c[g] = claim(p, nt_index_at(img[g], (uint32_t)p));
#pragma unroll
    for (int g = 0; g < kNtImages; ++g) v[g] = ld(p, nt_index_at(img[g], (uint32_t)p));
#pragma unroll
    for (int g = 0; g < kNtImages; ++g) {
      if (c[g] == 0u) continue;
      const uint32_t idx = nt_index_at(img[g], (uint32_t)p);
      st(p, idx, v[g] + nt_sync_step(take(p, idx), c[g], lr));
    }
  }
}

// ------------------------------------------------------------------------------------------
// ONE-LEVEL EXPECTIMAX over the spawn, for both afterstate families (q2048_av_search_*, q2048_nt_search_*): the row
// a player hands to play_action is, instead of q_a = score_a + v(c_a),
//   Q_a = (float)score_a + E_a,   E_a = the mean of best(s') over the spawns s' of the afterstate c_a.
// For a state s and a = 0..3, with c_a, score_a and legal_a the family's (move(), without the spawn):
//   a not legal:  Q_a = 0.0f, nothing is evaluated for it.
//   a legal:      c_a has n >= 1 empty cells (n <= 15).  For each empty cell j of c_a, ascending row-major:
//                   b2_j = best(c_a with a 2 at j), b4_j = best(c_a with a 4 at j)   (best: av_best of the family's
//                   evaluation -- q at the first maximum over the legal moves, 0.0f for a state without a move)
//                   t_j = 9.0 * (double)b2_j + (double)b4_j      (the product is exact, an fma gives the same t_j)
//                 S_a = ((0.0 + t_j0) + t_j1) + ...              double additions, in exactly this order
//                 E_a = (float)(S_a / (double)(10 * n))          one IEEE double division, rounded to float32 once
//                 Q_a = (float)score_a + E_a                     av_q
// The weights 9 : 1 stand for the env's spawn rule (draw_is_four: a 4 for x >= 3865470567, probability
// 0.1 - 0.6 * 2^-32); that 2^-32-sized difference from the integer threshold is ignored.
// A state has at most 4 * 15 * 2 = 120 chance nodes; they have FIXED SLOTS, slot = a * 32 + j * 2 + tile (tile 0: a
// 2, tile 1: a 4), 128 in all.  The CPU twin walks them serially; the device gives a wave to a state and spreads
// the live nodes over its lanes (q2048_kernels.hip).  Both sum through search_row, so the order of the S_a sums is the same.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kSearchSlots = 128u;
// The chance node of a slot: false when the slot holds none (its move is illegal or its cell is not empty in c_a;
// `node` is then meaningless).  One move per slot, not the four afterstates kept side by side.
Q_HD bool search_node(const Board& s, uint32_t slot, Board& node) {
  node = s;
  uint32_t score;
  const bool legal = move(node, (int)(slot >> 5), score);
  const uint32_t j = (slot >> 1) & 15u;
  const bool live = legal && ((empty_mask(node) >> j) & 1u) != 0u;
  put_cell(node, j, 1u + (slot & 1u));
  return live;
}
// The searched row of s.  best_at(slot, node) = best of the chance node in that slot; it is called for the live
// slots only, in ascending slot order.  (The four moves are a loop with selects, as in nt_eval.)
struct SearchEval { Row q; uint32_t legal; };
template <class BestAt>
Q_HD SearchEval search_row(const Board& s, BestAt best_at) {
  Q2048_NO_CONTRACT
  SearchEval ev{Row{0.0f, 0.0f, 0.0f, 0.0f}, 0u};
#pragma unroll 1
  for (int a = 0; a < 4; ++a) {
    Board c = s;
    uint32_t score;
    if (!move(c, a, score)) continue;
    ev.legal |= 1u << a;
    const uint32_t em = empty_mask(c);
    double sum = 0.0;
#pragma unroll 1
    for (uint32_t m = em; m != 0u; m &= m - 1u) {
      const uint32_t j = (uint32_t)__builtin_ctz(m), slot = (uint32_t)a * 32u + j * 2u;
      Board n2 = c, n4 = c;
      put_cell(n2, j, 1u);
      put_cell(n4, j, 2u);
      const float b2 = best_at(slot, n2);
      const float b4 = best_at(slot + 1u, n4);
      const double t = 9.0 * (double)b2 + (double)b4;
      sum = sum + t;
    }
    const float q = av_q(score, (float)(sum / (double)(10u * popc(em))));
    ev.q.q0 = a == 0 ? q : ev.q.q0;
    ev.q.q1 = a == 1 ? q : ev.q.q1;
    ev.q.q2 = a == 2 ? q : ev.q.q2;
    ev.q.q3 = a == 3 ? q : ev.q.q3;
  }
  return ev;
}

// ------------------------------------------------------------------------------------------
// TWO-LEVEL EXPECTIMAX (q2048_{av,nt}_search_*_depth with depth 2).  Write best_0 for the family's best above.  For
// d >= 1 the depth-d row of a state s is the searched row above with best_{d-1} in place of best:
//   a not legal:  Q^d_a = 0.0f, nothing is evaluated for it.
//   a legal:      for each empty cell j of c_a, ascending row-major:
//                   t_j = 9.0 * (double)best_{d-1}(c_a + 2 at j) + (double)best_{d-1}(c_a + 4 at j)
//                 S_a = ((0.0 + t_j0) + t_j1) + ...,  E_a = (float)(S_a / (double)(10 n)),  Q^d_a = (float)score_a + E_a
//   best_d(x) = av_best on the depth-d row of x: Q^d at the first maximum over the legal moves of x, 0.0f for a state
//               without a legal move -- nothing is evaluated beneath such a state.
// Depth 1 is search_row with the family's best, bit for bit.  Depth 2 is search_row whose best_at is search_best_of the
// search_row of the node: at most 120 level-one nodes with at most 120 leaves each, 14,400 family evaluations.  The
// order of every S sum, at BOTH levels, is search_row's: the device spreads the level-one nodes of a board over the waves
// of a block and the leaves of a node over the lanes of a wave, and sums each level through search_row.
// ------------------------------------------------------------------------------------------
// best_d(x) from the depth-d row of x
Q_HD float search_best_of(const SearchEval& ev) { return av_best(ev.legal, ev.q); }
// The depth-2 row of s.  best(x) = the family's best_0.
template <class Best>
Q_HD SearchEval search_row2(const Board& s, Best best) {
  return search_row(s, [&best](uint32_t, const Board& node) {
    return search_best_of(search_row(node, [&best](uint32_t, const Board& leaf) { return best(leaf); }));
  });
}

}  // namespace q2048
