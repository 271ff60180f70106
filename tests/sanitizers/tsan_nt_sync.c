/* Sanitizer driver for the synchronous batch step on the CPU twin (2048_q-learning_amd/csrc/q2048_host.cpp):
 * q2048_nt_sync_fused_rollout and q2048_nt_sync_update with 1 and 4 threads (Q2048_HOST_THREADS), a batch with a ragged
 * end (6501 boards: the twin gives a thread at least 2048 boards' worth of work, so four threads really run, over ranges
 * of unequal length, and really meet on the hot entries of acc) and launches of 1 + 2 + 9 steps.  A stand-alone program
 * -- build it with the twin's sources, once per sanitizer, and run it directly:
 *   gcc -O1 -g -std=c11 -fsanitize=thread -I include -c -o /tmp/nt_sync.o tests/sanitizers/tsan_nt_sync.c
 *   g++ -O1 -g -std=c++17 -fsanitize=thread -ffp-contract=off -fno-omit-frame-pointer -w -I include \
 *       -I 2048_q-learning_amd/csrc -pthread -o /tmp/nt_sync_tsan /tmp/nt_sync.o 2048_q-learning_amd/csrc/q2048_host.cpp
 *   TSAN_OPTIONS=halt_on_error=1 /tmp/nt_sync_tsan
 * and the same two lines with -fsanitize=address,undefined -fno-sanitize-recover=undefined for -fsanitize=thread:
 *   ASAN_OPTIONS=abort_on_error=1 /tmp/nt_sync_asan
 * V (exactly 4 * 16777216 floats), acc (exactly 4 * 16777216 * 2 words), pend (exactly B words), boards, aux, actions and
 * flags sit in allocations of exactly their sizes, so a read or write past either end -- a lane past the batch, an entry
 * past its table, a pair past acc -- is reported; the thread sanitizer reports an access to V, acc or pend that the
 * join between the phases does not order and that is not atomic.  Exits 0 when acc and pend are all zero after every
 * call, values have moved and are finite, every step is counted, and 1 thread and 4 threads give the same bits in V,
 * boards, aux and the integer statistics. */
#define _POSIX_C_SOURCE 200809L
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "q2048.h"

#define CHECK(x) do { int e_ = (x); if (e_ != 0) { fprintf(stderr, "%s -> %s\n", #x, q2048_strerror(e_)); return 2; } } while (0)

enum { B = 6501, STEPS = 12, ENTRIES = 4 * 16777216 };
static const int64_t cuts[3] = {1, 2, 9};

/* 16-byte aligned and exactly `size` bytes (aligned_alloc wants a multiple of the alignment: B words are not one) */
static void *alloc16(size_t size) {
  void *p = NULL;
  return posix_memalign(&p, 16, size) == 0 ? p : NULL;
}

static int all_zero(const uint64_t *w, size_t n) {
  uint64_t any = 0;
  for (size_t i = 0; i < n; ++i) any |= w[i];
  return any == 0;
}

/* twelve fused steps from fresh boards and a zeroed V, then one four-call step on the boards reached */
static int run(const char *threads, float *v, uint64_t *acc, uint64_t *pend, uint8_t *boards, q2048_aux *aux, int64_t *si) {
  double sf[Q2048_NSTAT_F] = {0};
  uint32_t status = 0, ctr = 0;
  int bad = 0;
  setenv("Q2048_HOST_THREADS", threads, 1);
  memset(v, 0, sizeof(float) * ENTRIES);
  memset(pend, 0x5a, sizeof(uint64_t) * B);                                            /* ignored on entry */
  CHECK(q2048_env_init(boards, aux, B, 4, 9, 100, NULL));
  for (int k = 0; k < 3; ++k) {
    CHECK(q2048_nt_sync_fused_rollout(boards, aux, v, acc, pend, B, cuts[k], k == 1 ? 1.0 : 0.25, 0.5, 0.95, 9, 100, ctr,
                                      si, sf, &status, NULL));
    ctr += (uint32_t)cuts[k];
    bad |= !all_zero(acc, (size_t)ENTRIES * 2) || !all_zero(pend, B);
  }
  uint8_t *actions = malloc(B), *done = calloc(B, 1);
  CHECK(q2048_nt_choose(v, boards, B, 0.25, 9, 100, ctr, actions, NULL));
  for (int i = 0; i < B; ++i) {
    if (i % 5 == 4) actions[i] = 7;                                                   /* every fifth lane a bad action */
    done[i] = (uint8_t)(i % 7 == 0);
  }
  CHECK(q2048_nt_sync_update(v, acc, boards, actions, boards, done, B, 0.5, 0.95, &status, NULL));
  bad |= !all_zero(acc, (size_t)ENTRIES * 2);
  free(actions); free(done);
  if (bad) fprintf(stderr, "%s thread(s): acc or pend not all zero after a call\n", threads);
  return bad | (status != Q2048_STATUS_BAD_ACTION);
}

int main(void) {
  int bad = 0;
  float *v = alloc16(sizeof(float) * ENTRIES), *v1 = malloc(sizeof(float) * ENTRIES);
  uint64_t *acc = alloc16(sizeof(uint64_t) * 2 * ENTRIES), *pend = alloc16(sizeof(uint64_t) * B);
  uint8_t *boards = alloc16(B * 16), *b1 = malloc(B * 16);
  q2048_aux *aux = alloc16(B * sizeof(q2048_aux)), *a1 = malloc(B * sizeof(q2048_aux));
  int64_t s1[Q2048_NSTAT_I] = {0}, s4[Q2048_NSTAT_I] = {0}, moved = 0;
  memset(acc, 0, sizeof(uint64_t) * 2 * ENTRIES);                                      /* all zero on entry */
  bad |= run("1", v, acc, pend, boards, aux, s1);
  memcpy(v1, v, sizeof(float) * ENTRIES);
  memcpy(b1, boards, B * 16);
  memcpy(a1, aux, B * sizeof(q2048_aux));
  bad |= run("4", v, acc, pend, boards, aux, s4);
  if (memcmp(v1, v, sizeof(float) * ENTRIES) != 0 || memcmp(b1, boards, B * 16) != 0 ||
      memcmp(a1, aux, B * sizeof(q2048_aux)) != 0 || memcmp(s1, s4, sizeof s1) != 0) {
    fprintf(stderr, "1 thread and 4 threads differ\n");
    bad = 1;
  }
  bad |= s1[Q2048_ST_STEPS] != (int64_t)B * STEPS || s1[Q2048_ST_EXPLORE] <= 0 || s1[Q2048_ST_VALID] <= 0;
  for (size_t i = 0; i < (size_t)ENTRIES; ++i) { bad |= !isfinite(v[i]); moved += v[i] != 0.0f; }
  bad |= moved <= 0;
  printf("%s: %lld values moved, the same bits with 1 and 4 threads\n", bad ? "FAILED" : "ok", (long long)moved);
  free(v); free(v1); free(acc); free(pend); free(boards); free(b1); free(aux); free(a1);
  return bad ? 1 : 0;
}
