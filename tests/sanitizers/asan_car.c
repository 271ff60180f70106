/* Sanitizer driver for carousel shaping on the CPU twin (2048_q-learning_amd/csrc/q2048_host.cpp): q2048_car_fused_rollout
 * and q2048_car_commit with 1 and 4 threads (Q2048_HOST_THREADS), S = 3 with the thresholds 3 and 5 (the tiles 8 and 32,
 * which a learning run crosses within its first steps), a ring of 7 records per stage that wraps many times, a batch with
 * a ragged end (6501 boards: the twin gives a thread at least 2048 boards' worth of work, so four threads really run) and
 * launches of 40 + 1 + 80 steps with the commit after each.  A stand-alone program -- build it with the twin's sources and
 * run it directly:
 *   gcc -O1 -g -std=c11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -c \
 *       -o /tmp/car.o tests/sanitizers/asan_car.c
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
 *       -fno-omit-frame-pointer -w -I include -I 2048_q-learning_amd/csrc -pthread -o /tmp/car \
 *       /tmp/car.o 2048_q-learning_amd/csrc/q2048_host.cpp
 *   ASAN_OPTIONS=abort_on_error=1 /tmp/car
 * V, pool, counts, fresh, boards and aux sit in allocations of exactly their sizes, so a read or write past either end --
 * a record of a lane past the batch, a slot past the ring, a stage past the last -- is reported.  Exits 0 when one thread
 * gives the same bytes twice, every step is counted, the counts equal the non-empty records seen before each commit, the
 * commit leaves `fresh` zero, row 0 of the pool stays zero, every valid record holds a tile and zeros in bytes 24..31, and
 * both rings have wrapped. */
#define _POSIX_C_SOURCE 200809L
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "q2048.h"

#define CHECK(x) do { int e_ = (x); if (e_ != 0) { fprintf(stderr, "%s -> %s\n", #x, q2048_strerror(e_)); return 2; } } while (0)

enum { B = 6501, P = 7, S = 3, STAGE = 4 * 16777216, STEPS = 121 };
static const uint32_t SPEC = 0x53u;      /* thresholds 2^3 and 2^5 */
static const int64_t cuts[3] = {40, 1, 80};

static int run(const char *threads, float *v, uint8_t *boards, q2048_aux *aux, uint8_t *pool, uint64_t *counts,
               uint8_t *fresh, int64_t *si) {
  double sf[Q2048_NSTAT_F] = {0};
  uint32_t status = 0, ctr = 0;
  uint64_t seen[S] = {0};
  int bad = 0;
  setenv("Q2048_HOST_THREADS", threads, 1);
  memset(v, 0, sizeof(float) * STAGE * S);
  memset(pool, 0, (size_t)S * P * 32);
  memset(counts, 0, sizeof(uint64_t) * S);
  memset(fresh, 0, (size_t)S * B * 32);
  CHECK(q2048_env_init(boards, aux, B, 4, 9, 100, NULL));
  for (int k = 0; k < 3; ++k) {
    CHECK(q2048_car_fused_rollout(boards, aux, v, SPEC, pool, counts, fresh, P, B, cuts[k], 0.3, 0.1, 0.95, 9, 100, ctr, si,
                                  sf, &status, NULL));
    ctr += (uint32_t)cuts[k];
    for (int s = 0; s < S; ++s)
      for (int i = 0; i < B; ++i) {
        const uint8_t *rec = fresh + ((size_t)s * B + i) * 32;
        int tile = 0, tail = 0;
        for (int c = 0; c < 16; ++c) tile |= rec[c];
        for (int c = 24; c < 32; ++c) tail |= rec[c];
        seen[s] += tile != 0;
        bad |= tail != 0 || (s == 0 && tile != 0);
      }
    CHECK(q2048_car_commit(pool, counts, fresh, SPEC, P, B, NULL));
    for (size_t i = 0; i < (size_t)S * B * 32; ++i) bad |= fresh[i] != 0;
    for (int s = 0; s < S; ++s) bad |= counts[s] != seen[s];
  }
  for (int i = 0; i < P * 32; ++i) bad |= pool[i] != 0;                         /* row 0 */
  for (int s = 1; s < S; ++s)
    for (int j = 0; j < P; ++j) {
      const uint8_t *rec = pool + ((size_t)s * P + j) * 32;
      int tile = 0, tail = 0;
      for (int c = 0; c < 16; ++c) tile |= rec[c];
      for (int c = 24; c < 32; ++c) tail |= rec[c];
      bad |= tile == 0 || tail != 0 || counts[s] <= (uint64_t)P;
    }
  bad |= status != 0;
  return bad;
}

int main(void) {
  int bad = 0;
  const size_t n = (size_t)STAGE * S;
  float *v = aligned_alloc(16, sizeof(float) * n), *v1 = malloc(sizeof(float) * n);
  uint8_t *boards = aligned_alloc(16, B * 16), *b1 = malloc(B * 16);
  q2048_aux *aux = aligned_alloc(16, B * sizeof(q2048_aux));
  uint8_t *pool = aligned_alloc(16, (size_t)S * P * 32), *p1 = malloc((size_t)S * P * 32);
  uint8_t *fresh = aligned_alloc(16, (size_t)S * B * 32);
  uint64_t *counts = malloc(sizeof(uint64_t) * S), c1[S];
  int64_t s1[Q2048_NSTAT_I] = {0}, s1b[Q2048_NSTAT_I] = {0}, s4[Q2048_NSTAT_I] = {0};
  /* the argument checks: the spec, NULL, alignment, the ring */
  bad |= q2048_car_commit(NULL, NULL, NULL, 0x35u, 0, -1, NULL) != Q2048_ERR_RANGE;
  bad |= q2048_car_commit(pool, NULL, fresh, SPEC, P, B, NULL) != Q2048_ERR_NULL;
  bad |= q2048_car_commit(pool + 8, counts, fresh, SPEC, P, B, NULL) != Q2048_ERR_ALIGN;
  bad |= q2048_car_commit(pool, counts, fresh, SPEC, 0, B, NULL) != Q2048_ERR_SIZE;
  /* one thread, twice: sequential, so the same bytes */
  bad |= run("1", v, boards, aux, pool, counts, fresh, s1);
  memcpy(v1, v, sizeof(float) * n);
  memcpy(b1, boards, B * 16);
  memcpy(p1, pool, (size_t)S * P * 32);
  memcpy(c1, counts, sizeof c1);
  bad |= run("1", v, boards, aux, pool, counts, fresh, s1b);
  bad |= memcmp(v1, v, sizeof(float) * n) != 0 || memcmp(b1, boards, B * 16) != 0 || memcmp(s1, s1b, sizeof s1) != 0;
  bad |= memcmp(p1, pool, (size_t)S * P * 32) != 0 || memcmp(c1, counts, sizeof c1) != 0;
  if (bad) fprintf(stderr, "one thread: FAILED\n");
  /* four threads: racing stores into V, every lane its own records */
  bad |= run("4", v, boards, aux, pool, counts, fresh, s4);
  bad |= s1[Q2048_ST_STEPS] != (int64_t)B * STEPS || s4[Q2048_ST_STEPS] != (int64_t)B * STEPS;
  bad |= s1[Q2048_ST_EPISODES] <= 0 || s4[Q2048_ST_EPISODES] <= 0;
  printf("%s: %llu / %llu records committed to stages 1 / 2, %lld episodes, %lld steps\n", bad ? "FAILED" : "ok",
         (unsigned long long)counts[1], (unsigned long long)counts[2], (long long)s4[Q2048_ST_EPISODES],
         (long long)s4[Q2048_ST_STEPS]);
  free(v); free(v1); free(boards); free(b1); free(aux); free(pool); free(p1); free(fresh); free(counts);
  return bad ? 1 : 0;
}
