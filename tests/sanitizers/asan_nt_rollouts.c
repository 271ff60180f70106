/* Sanitizer driver for the 6-tuple afterstate network on the CPU twin (2048_q-learning_amd/csrc/q2048_host.cpp):
 * q2048_nt_value, q2048_nt_lookup, q2048_nt_choose, q2048_nt_update, q2048_nt_fused_rollout and q2048_nt_play_rollout,
 * with 1 and 4 threads (Q2048_HOST_THREADS), a batch with a ragged end, launches of 1 + 63 + 136 steps, both env
 * profiles of the player.  A stand-alone program -- build it with the twin's sources and run it directly:
 *   gcc -O1 -g -std=c11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -c \
 *       -o /tmp/nt_rollouts.o tests/sanitizers/asan_nt_rollouts.c
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
 *       -fno-omit-frame-pointer -w -I include -I 2048_q-learning_amd/csrc -pthread -o /tmp/nt_rollouts \
 *       /tmp/nt_rollouts.o 2048_q-learning_amd/csrc/q2048_host.cpp
 *   ASAN_OPTIONS=abort_on_error=1 /tmp/nt_rollouts
 * Boards, aux, values (exactly 4 * 16777216 floats, 256 MiB) and every per-lane array sit in allocations of exactly their
 * size, so a read or write past either end -- a pattern index of 4, an entry index past 2^24 - 1 -- is reported.  Exits
 * 0 when the read-only entry points leave the values bit-identical, 4 threads equal 1 thread wherever the lanes do not
 * race (everything but the learner's values), the learner moved values of ALL FOUR patterns, every step is counted and
 * episodes end. */
#define _POSIX_C_SOURCE 200809L
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "q2048.h"

#define CHECK(x) do { int e_ = (x); if (e_ != 0) { fprintf(stderr, "%s -> %s\n", #x, q2048_strerror(e_)); return 2; } } while (0)

enum { B = 1000, V_PATTERN = 16777216, V_FLOATS = 4 * V_PATTERN };
static const int64_t cuts[3] = {1, 63, 136};

static void fill_values(float *v) {
  uint32_t x = 12345u;
  for (size_t i = 0; i < V_FLOATS; ++i) {                 /* every entry different: a wrong index reads a wrong value */
    x = x * 1664525u + 1013904223u;
    v[i] = (float)(int32_t)(x >> 8) / 8388608.0f - 1.0f;
  }
}

/* the four-call loop: choose, step, update, reset -- 40 steps on arrays of exactly B records */
static int four_calls(const char *threads, float *v, uint8_t *boards, q2048_aux *aux, float *q, float *val) {
  uint8_t *next = aligned_alloc(16, B * 16), *actions = malloc(B), *done = malloc(B), *max_log2 = malloc(B);
  float *reward = malloc(sizeof(float) * B);
  uint32_t status = 0, env_status = 0;
  setenv("Q2048_HOST_THREADS", threads, 1);
  CHECK(q2048_env_init(boards, aux, B, 4, 9, 100, NULL));
  for (uint32_t t = 0; t < 40; ++t) {
    CHECK(q2048_nt_choose(v, boards, B, 0.25, 9, 100, t, actions, NULL));
    CHECK(q2048_env_step_to(boards, next, aux, actions, B, 4, 9, 100, t, 0, reward, done, max_log2, NULL, &env_status, NULL));
    CHECK(q2048_nt_update(v, boards, actions, next, done, B, 0.1, 0.95, &status, NULL));
    memcpy(boards, next, B * 16);
    CHECK(q2048_env_reset_ex(boards, aux, done, B, 4, 9, 100, 0, NULL));
  }
  CHECK(q2048_nt_lookup(v, boards, B, q, NULL));
  CHECK(q2048_nt_value(v, boards, B, val, NULL));
  free(next); free(actions); free(done); free(max_log2); free(reward);
  return status != 0 || env_status != 0;
}

static int learn(const char *threads, float *v, uint8_t *boards, q2048_aux *aux, int64_t *si, double lr) {
  double sf[Q2048_NSTAT_F] = {0};
  uint32_t status = 0, ctr = 0;
  setenv("Q2048_HOST_THREADS", threads, 1);
  CHECK(q2048_env_init(boards, aux, B, 4, 9, 100, NULL));
  for (int k = 0; k < 3; ++k) {
    CHECK(q2048_nt_fused_rollout(boards, aux, v, B, cuts[k], 0.25, lr, 0.95, 9, 100, ctr, si, sf, &status, NULL));
    ctr += (uint32_t)cuts[k];
  }
  return status != 0;
}

static int play(const char *threads, uint32_t flags, const float *v, uint8_t *boards, q2048_aux *aux, int64_t *si) {
  double sf[Q2048_NSTAT_F] = {0};
  uint32_t status = 0, ctr = 0;
  setenv("Q2048_HOST_THREADS", threads, 1);
  CHECK(q2048_env_init(boards, aux, B, 4, 9, 100, NULL));
  for (int k = 0; k < 3; ++k) {
    CHECK(q2048_nt_play_rollout(boards, aux, v, B, cuts[k], k == 1 ? 0.25 : 0.0, 9, 100, ctr, flags, si, sf, &status, NULL));
    ctr += (uint32_t)cuts[k];
  }
  return status != 0;
}

static int differs(const float *a, const float *b, size_t lo, size_t hi) {
  return memcmp(a + lo, b + lo, sizeof(float) * (hi - lo)) != 0;
}
static int every_pattern_differs(const float *a, const float *b) {
  int all = 1;
  for (size_t p = 0; p < 4; ++p) all &= differs(a, b, p * V_PATTERN, (p + 1) * V_PATTERN);
  return all;
}

int main(void) {
  int bad = 0;
  float *v = aligned_alloc(16, sizeof(float) * V_FLOATS), *v0 = malloc(sizeof(float) * V_FLOATS);
  fill_values(v);
  memcpy(v0, v, sizeof(float) * V_FLOATS);
  uint8_t *b1 = aligned_alloc(16, B * 16), *b4 = aligned_alloc(16, B * 16);
  q2048_aux *a1 = aligned_alloc(16, B * sizeof(q2048_aux)), *a4 = aligned_alloc(16, B * sizeof(q2048_aux));
  int64_t episodes = 0;

  /* 1. frozen values (lr = 0): the learner is a function of V, 4 threads == 1 thread, V bit-identical */
  {
    int64_t s1[Q2048_NSTAT_I] = {0}, s4[Q2048_NSTAT_I] = {0};
    bad |= learn("1", v, b1, a1, s1, 0.0);
    bad |= learn("4", v, b4, a4, s4, 0.0);
    bad |= memcmp(b1, b4, B * 16) != 0 || memcmp(a1, a4, B * sizeof(q2048_aux)) != 0 || memcmp(s1, s4, sizeof s1) != 0;
    bad |= s4[Q2048_ST_STEPS] != (int64_t)B * 200 || s4[Q2048_ST_EPISODES] <= 0 || s4[Q2048_ST_EXPLORE] <= 0;
    bad |= differs(v, v0, 0, V_FLOATS);
    if (bad) fprintf(stderr, "frozen learner: mismatch\n");
  }
  /* 2. the player, four profiles: 4 threads == 1 thread, V bit-identical */
  const uint32_t profiles[4] = {0u, Q2048_FLAG_ENV_DQN, Q2048_FLAG_RESET_SHAPING, Q2048_FLAG_ENV_DQN | Q2048_FLAG_RESET_SHAPING};
  for (int p = 0; p < 4; ++p) {
    int64_t s1[Q2048_NSTAT_I] = {0}, s4[Q2048_NSTAT_I] = {0};
    bad |= play("1", profiles[p], v, b1, a1, s1);
    bad |= play("4", profiles[p], v, b4, a4, s4);
    bad |= memcmp(b1, b4, B * 16) != 0 || memcmp(a1, a4, B * sizeof(q2048_aux)) != 0 || memcmp(s1, s4, sizeof s1) != 0;
    bad |= s4[Q2048_ST_STEPS] != (int64_t)B * 200 || s4[Q2048_ST_EPISODES] <= 0 || s4[Q2048_ST_EXPLORE] <= 0 ||
           s4[Q2048_ST_INSERTS] != 0 || s4[Q2048_ST_DROPS] != 0;
    episodes += s4[Q2048_ST_EPISODES];
  }
  bad |= differs(v, v0, 0, V_FLOATS);
  if (bad) fprintf(stderr, "player: mismatch\n");
  /* 3. the learner learning, 4 threads (the lanes race on V by design: last writer wins), then the four-call loop */
  {
    int64_t s4[Q2048_NSTAT_I] = {0};
    float *q = aligned_alloc(16, sizeof(float) * 4 * B), *val = aligned_alloc(16, sizeof(float) * B);
    bad |= learn("4", v, b4, a4, s4, 0.1);
    bad |= s4[Q2048_ST_STEPS] != (int64_t)B * 200 || !every_pattern_differs(v, v0);
    memcpy(v0, v, sizeof(float) * V_FLOATS);
    bad |= four_calls("4", v, b4, a4, q, val);
    bad |= !every_pattern_differs(v, v0);
    bad |= four_calls("1", v, b1, a1, q, val);
    for (int i = 0; i < 4 * B; ++i) bad |= !(q[i] == q[i]);
    for (int i = 0; i < B; ++i) bad |= !(val[i] == val[i]);
    free(q); free(val);
    if (bad) fprintf(stderr, "learning: mismatch\n");
  }
  free(b1); free(b4); free(a1); free(a4); free(v); free(v0);
  printf("%s: %lld episodes played\n", bad ? "FAILED" : "ok", (long long)episodes);
  return bad ? 1 : 0;
}
