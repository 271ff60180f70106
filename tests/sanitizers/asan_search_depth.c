/* Sanitizer driver for the expectimax with a depth of the two afterstate families on the CPU twin
 * (2048_q-learning_amd/csrc/q2048_host.cpp): q2048_av_search_lookup_depth, q2048_av_search_play_rollout_depth,
 * q2048_nt_search_lookup_depth and q2048_nt_search_play_rollout_depth at depth 1 and 2, with 1 and 4 threads
 * (Q2048_HOST_THREADS), a batch with a ragged end (6501 boards: the twin gives a thread at least 2048 boards' worth of
 * work, so four threads really run, over ranges of unequal length), launches of 1 + 2 steps with exploration in the
 * second, both env profiles.
 * A stand-alone program -- build it with the twin's sources and run it directly:
 *   gcc -O1 -g -std=c11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -c \
 *       -o /tmp/search_depth.o tests/sanitizers/asan_search_depth.c
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
 *       -fno-omit-frame-pointer -w -I include -I 2048_q-learning_amd/csrc -pthread -o /tmp/search_depth \
 *       /tmp/search_depth.o 2048_q-learning_amd/csrc/q2048_host.cpp
 *   ASAN_OPTIONS=abort_on_error=1 /tmp/search_depth
 * Boards, aux, both value arrays (exactly 8 * 65536 and 4 * 16777216 floats) and both outputs sit in allocations of
 * exactly their size, so a read or write past either end -- a node past the batch, an entry index past the array -- is
 * reported.  The boards are crowded (one to three empty cells), so that a depth-2 step has hundreds of leaves, not
 * 14,400, and games end inside the three steps.  Exits 0 when the values stay bit-identical, 4 threads equal 1 thread in
 * rows, masks, boards, aux and the integer statistics, depth 1 equals the entry points without a depth, depth 2 differs
 * from depth 1, a depth of 0 or 3 is refused, every step is counted and episodes end. */
#define _POSIX_C_SOURCE 200809L
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "q2048.h"

#define CHECK(x) do { int e_ = (x); if (e_ != 0) { fprintf(stderr, "%s -> %s\n", #x, q2048_strerror(e_)); return 2; } } while (0)

enum { B = 6501, STEPS = 3, AV_FLOATS = 8 * 65536, NT_FLOATS = 4 * 16777216 };
static const int64_t cuts[2] = {1, 2};

typedef int (*lookup_fn)(const float *, const uint8_t *, int64_t, float *, uint8_t *, void *);
typedef int (*lookup_depth_fn)(const float *, const uint8_t *, int64_t, int, float *, uint8_t *, void *);
typedef int (*play_fn)(uint8_t *, q2048_aux *, const float *, int64_t, int64_t, double, uint64_t, uint64_t, uint32_t, uint32_t,
                       int64_t *, double *, uint32_t *, void *);
typedef int (*play_depth_fn)(uint8_t *, q2048_aux *, const float *, int64_t, int64_t, int, double, uint64_t, uint64_t, uint32_t,
                             uint32_t, int64_t *, double *, uint32_t *, void *);

static uint32_t lcg(uint32_t *x) { *x = *x * 1664525u + 1013904223u; return *x >> 8; }

static void fill_values(float *v, size_t n) {
  uint32_t x = 12345u;
  for (size_t i = 0; i < n; ++i) v[i] = (float)(int32_t)lcg(&x) / 8388608.0f - 1.0f;   /* every entry different */
}

/* tiles 2..128 everywhere but in one to three cells; board 0 is full with no equal neighbours (no legal move) */
static void crowded(uint8_t *boards) {
  uint32_t x = 777u;
  for (int i = 0; i < B; ++i) {
    for (int c = 0; c < 16; ++c) boards[16 * i + c] = (uint8_t)(1u + lcg(&x) % 7u);
    for (int k = 0; k < 3; ++k) boards[16 * i + lcg(&x) % 16u] = 0;
  }
  for (int c = 0; c < 16; ++c) boards[c] = (uint8_t)(1 + (((c >> 2) + c) & 1));
}

/* depth 0: the entry point without a depth */
static int lookup(const char *threads, lookup_fn f, lookup_depth_fn fd, int depth, const float *v, float *q, uint8_t *legal) {
  uint8_t *boards = aligned_alloc(16, B * 16);
  setenv("Q2048_HOST_THREADS", threads, 1);
  crowded(boards);
  if (depth == 0) CHECK(f(v, boards, B, q, legal, NULL));
  else CHECK(fd(v, boards, B, depth, q, legal, NULL));
  free(boards);
  return 0;
}

static int play(const char *threads, play_fn f, play_depth_fn fd, int depth, uint32_t flags, const float *v, uint8_t *boards,
                q2048_aux *aux, int64_t *si) {
  double sf[Q2048_NSTAT_F] = {0};
  uint32_t status = 0, ctr = 0;
  setenv("Q2048_HOST_THREADS", threads, 1);
  CHECK(q2048_env_init(boards, aux, B, 4, 9, 100, NULL));
  crowded(boards);
  for (int k = 0; k < 2; ++k) {
    const double eps = k == 1 ? 0.25 : 0.0;
    if (depth == 0) CHECK(f(boards, aux, v, B, cuts[k], eps, 9, 100, ctr, flags, si, sf, &status, NULL));
    else CHECK(fd(boards, aux, v, B, cuts[k], depth, eps, 9, 100, ctr, flags, si, sf, &status, NULL));
    ctr += (uint32_t)cuts[k];
  }
  return status != 0;
}

static int family(const char *name, lookup_fn look, lookup_depth_fn look_d, play_fn roll, play_depth_fn roll_d, size_t floats,
                  int64_t *episodes) {
  int bad = 0;
  float *v = aligned_alloc(16, sizeof(float) * floats), *v0 = malloc(sizeof(float) * floats);
  fill_values(v, floats);
  memcpy(v0, v, sizeof(float) * floats);
  uint8_t *b1 = aligned_alloc(16, B * 16), *b4 = aligned_alloc(16, B * 16), *b0 = aligned_alloc(16, B * 16);
  q2048_aux *a1 = aligned_alloc(16, B * sizeof(q2048_aux)), *a4 = aligned_alloc(16, B * sizeof(q2048_aux));
  q2048_aux *a0 = aligned_alloc(16, B * sizeof(q2048_aux));
  /* 1. the rows and the masks: depth 1 == no depth; depth 2 with 4 threads == with 1 thread, and != depth 1 */
  {
    float *q0 = aligned_alloc(16, sizeof(float) * 4 * B), *q1 = aligned_alloc(16, sizeof(float) * 4 * B);
    float *q4 = aligned_alloc(16, sizeof(float) * 4 * B);
    uint8_t *l0 = malloc(B), *l1 = malloc(B), *l4 = malloc(B);
    int live = 0;
    bad |= lookup("4", look, look_d, 0, v, q0, l0);
    bad |= lookup("1", look, look_d, 1, v, q1, l1);
    bad |= lookup("4", look, look_d, 1, v, q4, l4);
    bad |= memcmp(q0, q1, sizeof(float) * 4 * B) != 0 || memcmp(l0, l1, B) != 0;
    bad |= memcmp(q0, q4, sizeof(float) * 4 * B) != 0 || memcmp(l0, l4, B) != 0;
    bad |= lookup("1", look, look_d, 2, v, q1, l1);
    bad |= lookup("4", look, look_d, 2, v, q4, l4);
    bad |= memcmp(q1, q4, sizeof(float) * 4 * B) != 0 || memcmp(l1, l4, B) != 0 || memcmp(l0, l4, B) != 0;
    bad |= memcmp(q0, q4, sizeof(float) * 4 * B) == 0;
    for (int i = 0; i < 4 * B; ++i) bad |= !(q4[i] == q4[i]);
    for (int i = 0; i < B; ++i) { bad |= l4[i] > 15; live += l4[i] != 0; }
    bad |= l4[0] != 0 || q4[0] != 0.0f || q4[1] != 0.0f || q4[2] != 0.0f || q4[3] != 0.0f || live < B / 2;
    /* a depth that is refused writes nothing: the rows keep their bytes */
    memcpy(q1, q4, sizeof(float) * 4 * B);
    bad |= look_d(v, b1, B, 0, q4, l4, NULL) != Q2048_ERR_RANGE || look_d(v, b1, B, 3, q4, l4, NULL) != Q2048_ERR_RANGE;
    bad |= memcmp(q1, q4, sizeof(float) * 4 * B) != 0;
    free(q0); free(q1); free(q4); free(l0); free(l1); free(l4);
    if (bad) fprintf(stderr, "%s: lookup mismatch\n", name);
  }
  /* 2. the player, both env profiles (the second with reset-shaping) */
  const uint32_t profiles[2] = {0u, Q2048_FLAG_ENV_DQN | Q2048_FLAG_RESET_SHAPING};
  for (int p = 0; p < 2; ++p) {
    int64_t s0[Q2048_NSTAT_I] = {0}, s1[Q2048_NSTAT_I] = {0}, s4[Q2048_NSTAT_I] = {0};
    bad |= play("4", roll, roll_d, 0, profiles[p], v, b0, a0, s0);
    bad |= play("1", roll, roll_d, 1, profiles[p], v, b1, a1, s1);
    bad |= memcmp(b0, b1, B * 16) != 0 || memcmp(a0, a1, B * sizeof(q2048_aux)) != 0 || memcmp(s0, s1, sizeof s1) != 0;
    memset(s1, 0, sizeof s1);
    bad |= play("1", roll, roll_d, 2, profiles[p], v, b1, a1, s1);
    bad |= play("4", roll, roll_d, 2, profiles[p], v, b4, a4, s4);
    bad |= memcmp(b1, b4, B * 16) != 0 || memcmp(a1, a4, B * sizeof(q2048_aux)) != 0 || memcmp(s1, s4, sizeof s1) != 0;
    bad |= memcmp(b0, b4, B * 16) == 0;
    bad |= s4[Q2048_ST_STEPS] != (int64_t)B * STEPS || s4[Q2048_ST_EPISODES] <= 0 || s4[Q2048_ST_EXPLORE] <= 0 ||
           s4[Q2048_ST_INSERTS] != 0 || s4[Q2048_ST_DROPS] != 0;
    *episodes += s4[Q2048_ST_EPISODES];
    if (bad) fprintf(stderr, "%s: player mismatch (profile %d)\n", name, p);
  }
  {
    uint32_t status = 0;
    memcpy(b0, b4, B * 16);
    bad |= roll_d(b4, a4, v, B, 1, 3, 0.0, 9, 100, 0, 0, NULL, NULL, &status, NULL) != Q2048_ERR_RANGE;
    bad |= roll_d(b4, a4, v, B, 1, -1, 0.0, 9, 100, 0, 0, NULL, NULL, &status, NULL) != Q2048_ERR_RANGE;
    bad |= memcmp(b0, b4, B * 16) != 0;
  }
  bad |= memcmp(v, v0, sizeof(float) * floats) != 0;
  if (bad) fprintf(stderr, "%s: FAILED\n", name);
  free(b0); free(b1); free(b4); free(a0); free(a1); free(a4); free(v); free(v0);
  return bad;
}

int main(void) {
  int64_t episodes = 0;
  int bad = family("afterstate", q2048_av_search_lookup, q2048_av_search_lookup_depth, q2048_av_search_play_rollout,
                   q2048_av_search_play_rollout_depth, AV_FLOATS, &episodes);
  bad |= family("ntuple", q2048_nt_search_lookup, q2048_nt_search_lookup_depth, q2048_nt_search_play_rollout,
                q2048_nt_search_play_rollout_depth, NT_FLOATS, &episodes);
  printf("%s: %lld episodes played\n", bad ? "FAILED" : "ok", (long long)episodes);
  return bad ? 1 : 0;
}
