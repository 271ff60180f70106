/* Sanitizer driver for q2048_rt_play_rollout on the CPU twin (2048_q-learning_amd/csrc/q2048_host.cpp): the greedy
 * player on row-tuple weights, 4 threads (Q2048_HOST_THREADS), both env profiles with and without the reset-shaping
 * bit, a batch with a ragged end, launches of 1 + 63 + 136 steps.  A stand-alone program -- build it with the twin's
 * sources and run it directly:
 *   gcc -O1 -g -std=c11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -c \
 *       -o /tmp/rt_play.o tests/sanitizers/asan_rt_play_rollout.c
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
 *       -fno-omit-frame-pointer -w -I include -I 2048_q-learning_amd/csrc -pthread -o /tmp/rt_play /tmp/rt_play.o \
 *       2048_q-learning_amd/csrc/q2048_host.cpp
 *   ASAN_OPTIONS=abort_on_error=1 /tmp/rt_play
 * (-fsanitize=thread likewise).  Boards, aux and weights sit in allocations of exactly their size, so a read or
 * write past either end is reported.  Exits 0 when the weights are bit-identical afterwards, 4 threads equal 1
 * thread in boards, aux and the integer statistics, every step is counted and episodes end. */
#define _POSIX_C_SOURCE 200809L
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "q2048.h"

#define CHECK(x) do { int e_ = (x); if (e_ != 0) { fprintf(stderr, "%s -> %s\n", #x, q2048_strerror(e_)); return 2; } } while (0)

enum { B = 1000, W_FLOATS = 4 * 65536 * 4 };

static int play(const char *threads, uint32_t flags, const float *w, uint8_t *boards, q2048_aux *aux, int64_t *si) {
  static const int64_t cuts[3] = {1, 63, 136};
  double sf[Q2048_NSTAT_F] = {0};
  uint32_t status = 0, ctr = 0;
  setenv("Q2048_HOST_THREADS", threads, 1);
  CHECK(q2048_env_init(boards, aux, B, 4, 9, 100, NULL));
  for (int k = 0; k < 3; ++k) {
    CHECK(q2048_rt_play_rollout(boards, aux, w, B, cuts[k], k == 1 ? 0.25 : 0.0, 9, 100, ctr, flags, si, sf, &status, NULL));
    ctr += (uint32_t)cuts[k];
  }
  return status != 0;
}

int main(void) {
  int bad = 0;
  float *w = aligned_alloc(16, sizeof(float) * W_FLOATS), *w0 = malloc(sizeof(float) * W_FLOATS);
  uint32_t x = 12345u;
  for (size_t i = 0; i < W_FLOATS; ++i) {                 /* every entry different: a wrong index reads a wrong row */
    x = x * 1664525u + 1013904223u;
    w[i] = (float)(int32_t)(x >> 8) / 8388608.0f - 1.0f;
  }
  memcpy(w0, w, sizeof(float) * W_FLOATS);
  const uint32_t profiles[4] = {0u, Q2048_FLAG_ENV_DQN, Q2048_FLAG_RESET_SHAPING, Q2048_FLAG_ENV_DQN | Q2048_FLAG_RESET_SHAPING};
  int64_t episodes = 0;
  for (int p = 0; p < 4; ++p) {
    uint8_t *b1 = aligned_alloc(16, B * 16), *b4 = aligned_alloc(16, B * 16);
    q2048_aux *a1 = aligned_alloc(16, B * sizeof(q2048_aux)), *a4 = aligned_alloc(16, B * sizeof(q2048_aux));
    int64_t s1[Q2048_NSTAT_I] = {0}, s4[Q2048_NSTAT_I] = {0};
    bad |= play("1", profiles[p], w, b1, a1, s1);
    bad |= play("4", profiles[p], w, b4, a4, s4);
    bad |= memcmp(b1, b4, B * 16) != 0 || memcmp(a1, a4, B * sizeof(q2048_aux)) != 0 || memcmp(s1, s4, sizeof s1) != 0;
    bad |= s4[Q2048_ST_STEPS] != (int64_t)B * 200 || s4[Q2048_ST_EPISODES] <= 0 || s4[Q2048_ST_EXPLORE] <= 0 ||
           s4[Q2048_ST_INSERTS] != 0 || s4[Q2048_ST_DROPS] != 0;
    episodes += s4[Q2048_ST_EPISODES];
    free(b1); free(b4); free(a1); free(a4);
  }
  bad |= memcmp(w, w0, sizeof(float) * W_FLOATS) != 0;
  /* a refused call and the two no-ops touch nothing: the addresses below are not mapped */
  bad |= q2048_rt_play_rollout((uint8_t *)0x1000, (q2048_aux *)0x2000, (const float *)0x3000, 64, 1, 0.0, 1, 0, 0,
                               Q2048_FLAG_INDEPENDENT, NULL, NULL, (uint32_t *)0x4000, NULL) != Q2048_ERR_FLAGS;
  bad |= q2048_rt_play_rollout((uint8_t *)0x1000, (q2048_aux *)0x2000, (const float *)0x3000, 0, 1, 0.0, 1, 0, 0, 0u,
                               NULL, NULL, (uint32_t *)0x4000, NULL) != Q2048_OK;
  bad |= q2048_rt_play_rollout((uint8_t *)0x1000, (q2048_aux *)0x2000, (const float *)0x3000, 64, 0, 0.0, 1, 0, 0, 0u,
                               NULL, NULL, (uint32_t *)0x4000, NULL) != Q2048_OK;
  printf("rt player driver: %d envs x 200 steps x 4 profiles, 1 and 4 threads, %lld episodes: %s\n", B,
         (long long)episodes, bad ? "MISMATCH" : "weights untouched, 4 threads == 1 thread");
  free(w); free(w0);
  return bad;
}
