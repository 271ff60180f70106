/* Sanitizer driver for the temporal-coherence step sizes of the 6-tuple afterstate network on the CPU twin
 * (2048_q-learning_amd/csrc/q2048_host.cpp): q2048_nt_tc_update and q2048_nt_tc_fused_rollout, with 1 and 4 threads
 * (Q2048_HOST_THREADS), a batch with a ragged end (6501 boards: the twin gives a thread at least 2048 boards' worth of
 * work, so four threads really run, over ranges of unequal length, and really race on the hot entries) and launches of
 * 1 + 2 + 3 steps.  A stand-alone program -- build it with the twin's sources and run it directly:
 *   gcc -O1 -g -std=c11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -c \
 *       -o /tmp/nt_tc.o tests/sanitizers/asan_nt_tc.c
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
 *       -fno-omit-frame-pointer -w -I include -I 2048_q-learning_amd/csrc -pthread -o /tmp/nt_tc \
 *       /tmp/nt_tc.o 2048_q-learning_amd/csrc/q2048_host.cpp
 *   ASAN_OPTIONS=abort_on_error=1 /tmp/nt_tc
 * V (exactly 4 * 16777216 floats) and acc (exactly 4 * 16777216 * 2 floats) sit in allocations of exactly their sizes,
 * as do boards and aux, so a read or write past either end -- a lane past the batch, an entry or a pair past its
 * array -- is reported.  Exits 0 when every pair of acc is finite with A >= 0 and |E| <= A after every run, pairs and
 * values have moved, one thread gives the same bits twice, and every step is counted. */
#define _POSIX_C_SOURCE 200809L
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "q2048.h"

#define CHECK(x) do { int e_ = (x); if (e_ != 0) { fprintf(stderr, "%s -> %s\n", #x, q2048_strerror(e_)); return 2; } } while (0)

enum { B = 6501, STEPS = 6, ENTRIES = 4 * 16777216 };
static const int64_t cuts[3] = {1, 2, 3};

/* |E| <= A, A >= 0 and both finite for all 2^26 pairs; counts the pairs with a history */
static int coherent(const float *acc, int64_t *seen) {
  int bad = 0;
  *seen = 0;
  for (size_t i = 0; i < (size_t)ENTRIES; ++i) {
    const float E = acc[2 * i], A = acc[2 * i + 1];
    bad |= !(fabsf(E) <= A) || !(A >= 0.0f) || !isfinite(A);
    *seen += A > 0.0f;
  }
  return bad;
}

/* six fused steps from fresh boards and zeroed V and acc, then one four-call TD step on the boards reached */
static int run(const char *threads, float *v, float *acc, uint8_t *boards, q2048_aux *aux, int64_t *si) {
  double sf[Q2048_NSTAT_F] = {0};
  uint32_t status = 0, ctr = 0;
  setenv("Q2048_HOST_THREADS", threads, 1);
  memset(v, 0, sizeof(float) * ENTRIES);
  memset(acc, 0, sizeof(float) * 2 * ENTRIES);
  CHECK(q2048_env_init(boards, aux, B, 4, 9, 100, NULL));
  for (int k = 0; k < 3; ++k) {
    CHECK(q2048_nt_tc_fused_rollout(boards, aux, v, acc, B, cuts[k], k == 1 ? 0.25 : 1.0, 0.5, 0.95, 9, 100, ctr, si, sf,
                                    &status, NULL));
    ctr += (uint32_t)cuts[k];
  }
  uint8_t *actions = malloc(B), *done = calloc(B, 1);
  for (int i = 0; i < B; ++i) actions[i] = (uint8_t)(i % 5 == 4 ? 7 : i & 3);      /* every fifth lane a bad action */
  CHECK(q2048_nt_tc_update(v, acc, boards, actions, boards, done, B, 0.5, 0.95, &status, NULL));
  free(actions); free(done);
  return status != Q2048_STATUS_BAD_ACTION;
}

int main(void) {
  int bad = 0;
  float *v = aligned_alloc(16, sizeof(float) * ENTRIES), *acc = aligned_alloc(16, sizeof(float) * 2 * ENTRIES);
  float *v1 = malloc(sizeof(float) * ENTRIES), *acc1 = malloc(sizeof(float) * 2 * ENTRIES);
  uint8_t *boards = aligned_alloc(16, B * 16), *b1 = malloc(B * 16);
  q2048_aux *aux = aligned_alloc(16, B * sizeof(q2048_aux));
  int64_t seen = 0, seen4 = 0, moved = 0;
  int64_t s1[Q2048_NSTAT_I] = {0}, s1b[Q2048_NSTAT_I] = {0}, s4[Q2048_NSTAT_I] = {0};
  /* one thread, twice: sequential, so the same bits */
  bad |= run("1", v, acc, boards, aux, s1);
  bad |= coherent(acc, &seen);
  memcpy(v1, v, sizeof(float) * ENTRIES);
  memcpy(acc1, acc, sizeof(float) * 2 * ENTRIES);
  memcpy(b1, boards, B * 16);
  bad |= run("1", v, acc, boards, aux, s1b);
  bad |= memcmp(v1, v, sizeof(float) * ENTRIES) != 0 || memcmp(acc1, acc, sizeof(float) * 2 * ENTRIES) != 0 ||
         memcmp(b1, boards, B * 16) != 0 || memcmp(s1, s1b, sizeof s1) != 0;
  if (bad) fprintf(stderr, "one thread: FAILED\n");
  /* four threads: racing stores, the invariant holds all the same */
  bad |= run("4", v, acc, boards, aux, s4);
  bad |= coherent(acc, &seen4);
  for (size_t i = 0; i < (size_t)ENTRIES; ++i) { bad |= !isfinite(v[i]); moved += v[i] != 0.0f; }
  bad |= seen <= 0 || seen4 <= 0 || moved <= 0;
  bad |= s1[Q2048_ST_STEPS] != (int64_t)B * STEPS || s4[Q2048_ST_STEPS] != (int64_t)B * STEPS;
  bad |= s1[Q2048_ST_EXPLORE] <= 0 || s4[Q2048_ST_EXPLORE] <= 0 || s1[Q2048_ST_VALID] <= 0 || s4[Q2048_ST_VALID] <= 0;
  printf("%s: %lld / %lld pairs with a history (1 / 4 threads), %lld values moved, %lld steps\n", bad ? "FAILED" : "ok",
         (long long)seen, (long long)seen4, (long long)moved, (long long)s4[Q2048_ST_STEPS]);
  free(v); free(acc); free(v1); free(acc1); free(boards); free(b1); free(aux);
  return bad ? 1 : 0;
}
