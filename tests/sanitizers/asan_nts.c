/* Sanitizer driver for the staged 6-tuple network on the CPU twin (2048_q-learning_amd/csrc/q2048_host.cpp): the nine
 * q2048_nts_* functions with 1 and 4 threads (Q2048_HOST_THREADS), S = 2 with the threshold 4 (the tile 16, which a
 * learning run reaches within its first steps), a batch with a ragged end (6501 boards: the twin gives a thread at
 * least 2048 boards' worth of work, so four threads really run and really race on the hot entries) and launches of
 * 1 + 2 + 3 steps.  A stand-alone program -- build it with the twin's sources and run it directly:
 *   gcc -O1 -g -std=c11 -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include -c \
 *       -o /tmp/nts.o tests/sanitizers/asan_nts.c
 *   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -ffp-contract=off \
 *       -fno-omit-frame-pointer -w -I include -I 2048_q-learning_amd/csrc -pthread -o /tmp/nts \
 *       /tmp/nts.o 2048_q-learning_amd/csrc/q2048_host.cpp
 *   ASAN_OPTIONS=abort_on_error=1 /tmp/nts
 * V (exactly 2 * 4 * 16777216 floats) sits in an allocation of exactly its size, as do boards, aux and every output, so
 * a read or write past either end -- a lane past the batch, an entry past the last stage -- is reported.  Exits 0 when
 * the values stay finite, both stages have moved, one thread gives the same bits twice, every step is counted, the
 * readers agree with each other (value of a board = the lookup's row minus the score where the move is illegal), and a
 * promotion leaves no entry of stage 1 zero where stage 0 is not. */
#define _POSIX_C_SOURCE 200809L
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "q2048.h"

#define CHECK(x) do { int e_ = (x); if (e_ != 0) { fprintf(stderr, "%s -> %s\n", #x, q2048_strerror(e_)); return 2; } } while (0)

enum { B = 6501, STEPS = 6, STAGE = 4 * 16777216, STAGES_N = 2, SEARCH_B = 37, SEARCH2_B = 3 };
static const uint32_t SPEC = 4u;      /* one threshold: the tile 2^4 */
static const int64_t cuts[3] = {1, 2, 3};

/* six fused steps from fresh boards and zeroed tables, one four-call TD step, then every reader and both players */
static int run(const char *threads, float *v, uint8_t *boards, q2048_aux *aux, int64_t *si) {
  double sf[Q2048_NSTAT_F] = {0};
  int64_t pi[Q2048_NSTAT_I] = {0};
  double pf[Q2048_NSTAT_F] = {0};
  uint32_t status = 0, ctr = 0;
  int bad = 0;
  setenv("Q2048_HOST_THREADS", threads, 1);
  memset(v, 0, sizeof(float) * STAGE * STAGES_N);
  CHECK(q2048_env_init(boards, aux, B, 4, 9, 100, NULL));
  for (int k = 0; k < 3; ++k) {
    CHECK(q2048_nts_fused_rollout(boards, aux, v, SPEC, B, cuts[k], k == 1 ? 0.25 : 1.0, 0.5, 0.95, 9, 100, ctr, si, sf,
                                  &status, NULL));
    ctr += (uint32_t)cuts[k];
  }
  uint8_t *actions = malloc(B), *done = calloc(B, 1), *legal = malloc(B);
  float *q = aligned_alloc(16, sizeof(float) * 4 * B), *val = aligned_alloc(16, sizeof(float) * ((B + 3) & ~3));
  for (int i = 0; i < B; ++i) actions[i] = (uint8_t)(i % 5 == 4 ? 7 : i & 3);      /* every fifth lane a bad action */
  CHECK(q2048_nts_update(v, SPEC, boards, actions, boards, done, B, 0.5, 0.95, &status, NULL));
  bad |= status != Q2048_STATUS_BAD_ACTION;
  CHECK(q2048_nts_value(v, SPEC, boards, B, val, NULL));
  CHECK(q2048_nts_lookup(v, SPEC, boards, B, q, NULL));
  CHECK(q2048_nts_choose(v, SPEC, boards, B, 0.3, 9, 100, ctr, actions, NULL));
  CHECK(q2048_legal_moves(boards, B, 4, legal, NULL));
  for (int i = 0; i < B; ++i) {
    bad |= actions[i] > 3 || !isfinite(val[i]);
    for (int a = 0; a < 4; ++a)      /* an illegal move leaves the board: q_a = 0 + v(board), bit for bit */
      if (!((legal[i] >> a) & 1)) bad |= memcmp(&q[4 * i + a], &val[i], sizeof(float)) != 0;
  }
  /* the searched rows, then the three players on copies of the boards */
  CHECK(q2048_nts_search_lookup_depth(v, SPEC, boards, SEARCH_B, 1, q, legal, NULL));
  CHECK(q2048_nts_search_lookup_depth(v, SPEC, boards, SEARCH2_B, 2, q, legal, NULL));
  for (int i = 0; i < 4 * SEARCH2_B; ++i) bad |= !isfinite(q[i]);
  uint8_t *pb = aligned_alloc(16, B * 16);
  q2048_aux *pa = aligned_alloc(16, B * sizeof(q2048_aux));
  memcpy(pb, boards, B * 16); memcpy(pa, aux, B * sizeof(q2048_aux));
  CHECK(q2048_nts_play_rollout(pb, pa, v, SPEC, B, 5, 0.1, 9, 100, ctr, Q2048_FLAG_ENV_DQN, pi, pf, &status, NULL));
  CHECK(q2048_nts_search_play_rollout_depth(pb, pa, v, SPEC, SEARCH_B, 3, 1, 0.1, 9, 100, ctr + 5, 0, pi, pf, &status, NULL));
  CHECK(q2048_nts_search_play_rollout_depth(pb, pa, v, SPEC, SEARCH2_B, 1, 2, 0.0, 9, 100, ctr + 8, Q2048_FLAG_RESET_SHAPING,
                                            pi, pf, &status, NULL));
  bad |= pi[Q2048_ST_STEPS] != (int64_t)B * 5 + SEARCH_B * 3 + SEARCH2_B;
  free(actions); free(done); free(legal); free(q); free(val); free(pb); free(pa);
  return bad;
}

int main(void) {
  int bad = 0;
  const size_t n = (size_t)STAGE * STAGES_N;
  float *v = aligned_alloc(16, sizeof(float) * n), *v1 = malloc(sizeof(float) * n);
  uint8_t *boards = aligned_alloc(16, B * 16), *b1 = malloc(B * 16);
  q2048_aux *aux = aligned_alloc(16, B * sizeof(q2048_aux));
  int64_t s1[Q2048_NSTAT_I] = {0}, s1b[Q2048_NSTAT_I] = {0}, s4[Q2048_NSTAT_I] = {0};
  int64_t moved[STAGES_N] = {0}, copied = -1, again = -1, left = 0;
  /* the argument checks: a malformed spec before everything else, the stage numbers of a promotion */
  bad |= q2048_nts_value(NULL, 0x35u, NULL, -1, NULL, NULL) != Q2048_ERR_RANGE;
  bad |= q2048_nts_promote(v, 0x10000003u, 0, 1, NULL, NULL) != Q2048_ERR_RANGE;
  bad |= q2048_nts_promote(v, SPEC, 0, 0, NULL, NULL) != Q2048_ERR_RANGE || q2048_nts_promote(v, SPEC, 0, 2, NULL, NULL) != Q2048_ERR_RANGE;
  bad |= q2048_nts_promote(NULL, SPEC, 0, 1, NULL, NULL) != Q2048_ERR_NULL;
  /* one thread, twice: sequential, so the same bits */
  bad |= run("1", v, boards, aux, s1);
  memcpy(v1, v, sizeof(float) * n);
  memcpy(b1, boards, B * 16);
  bad |= run("1", v, boards, aux, s1b);
  bad |= memcmp(v1, v, sizeof(float) * n) != 0 || memcmp(b1, boards, B * 16) != 0 || memcmp(s1, s1b, sizeof s1) != 0;
  if (bad) fprintf(stderr, "one thread: FAILED\n");
  /* four threads: racing stores */
  bad |= run("4", v, boards, aux, s4);
  for (int k = 0; k < STAGES_N; ++k)
    for (size_t i = 0; i < (size_t)STAGE; ++i) { bad |= !isfinite(v[(size_t)k * STAGE + i]); moved[k] += v[(size_t)k * STAGE + i] != 0.0f; }
  bad |= moved[0] <= 0 || moved[1] <= 0;
  bad |= s1[Q2048_ST_STEPS] != (int64_t)B * STEPS || s4[Q2048_ST_STEPS] != (int64_t)B * STEPS;
  bad |= s1[Q2048_ST_EXPLORE] <= 0 || s4[Q2048_ST_EXPLORE] <= 0 || s1[Q2048_ST_VALID] <= 0 || s4[Q2048_ST_VALID] <= 0;
  /* promotion with 4 threads and with 1: afterwards no entry of stage 1 is zero where stage 0 is not */
  if (q2048_nts_promote(v, SPEC, 0, 1, &copied, NULL) != 0) bad = 1;
  setenv("Q2048_HOST_THREADS", "1", 1);
  if (q2048_nts_promote(v, SPEC, 0, 1, &again, NULL) != 0 || q2048_nts_promote(v, SPEC, 0, 1, NULL, NULL) != 0) bad = 1;
  for (size_t i = 0; i < (size_t)STAGE; ++i) {
    uint32_t d, s;
    memcpy(&d, &v[STAGE + i], 4); memcpy(&s, &v[i], 4);
    left += d == 0 && s != 0;
  }
  bad |= copied <= 0 || again != 0 || left != 0;
  printf("%s: %lld / %lld values moved in stage 0 / 1, %lld promoted, %lld steps\n", bad ? "FAILED" : "ok",
         (long long)moved[0], (long long)moved[1], (long long)copied, (long long)s4[Q2048_ST_STEPS]);
  free(v); free(v1); free(boards); free(b1); free(aux);
  return bad ? 1 : 0;
}
