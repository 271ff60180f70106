/*
 * q2048.h -- C ABI of libq2048_hip.so: the MI355X (gfx950) hot path of the batched 2048
 * tabular Q-learning loop.
 *
 * This is the drop-in boundary for the path of Rocco9999/2048_Q-Learning named by
 * BASELINE.json: QLearningBase/environment/Game2048_env.py (Game2048_env.step/reset) and
 * QLearningBase/Agent/main.py (QLearningAgent.choose_action/update_q_value).  The reference is
 * pure Python and has no FFI; these are the entry points a binding for that path needs
 * (INTEGRATION.md shows the ctypes stub).  Every function below names the reference
 * interface it replaces.
 *
 * Conventions
 *   - Plain pointers and sizes only.  Every data pointer is a DEVICE pointer (HIP); the caller
 *     owns all memory -- the library allocates nothing, with one exception the caller asks for by
 *     name: q2048_table_alloc / _reserve / _grow* / _trim / _free (a Q-table mapped from small physical
 *     chunks, which may grow; _alloc, _reserve, _grow and _free are host-synchronous, _grow_begin and
 *     _grow_commit return at once).  `stream` is a hipStream_t (NULL = default stream).  All other
 *     calls are asynchronous and stream-ordered: no host synchronisation inside.
 *   - The same ABI exists for HOST memory: libq2048_host.so (csrc/q2048_host.cpp), compiled from the same
 *     per-lane arithmetic and table layout -- every pointer is then a host pointer, `stream` is ignored and every
 *     call is complete when it returns; the chunk allocator returns Q2048_ERR_UNSUPPORTED there.  It is a
 *     device of its own ("cpu"), loaded only when asked for by name, never a fallback.
 *   - boards   uint8_t[B][16]: 4x4 board, row-major, log2 tiles (0 empty, k = tile 2^k), the
 *              device image of the reference's np.int64[4,4] raw-value board
 *              (Game2048_env.py:12).  16-byte aligned.
 *   - aux      q2048_aux[B]: per-env state that Game2048_env keeps in Python attributes
 *              (Game2048_env.py:81-95).  16-byte aligned.
 *   - table    q2048_slot[1 << cap_log2]: open-addressed hash Q-table, the device form of
 *              `defaultdict(lambda: np.zeros(4))` (Agent/main.py:16).  Zero-filled = empty.
 *              16-byte aligned; 128-byte alignment makes every group of four slots one memory
 *              line, which is what the bucketised probe sequence is built for.
 *   - RNG      counter based: draws = Philox4x32-10(key = seed, counter = (global env id,
 *              step counter ctr, stream)); lane i has global env id env_id0 + i, so results do
 *              not depend on how a batch is sharded over GPUs.
 *   - return   0 on success, a negative Q2048_ERR_* otherwise (argument errors are detected
 *              on the host before anything is launched).  Data-dependent conditions are
 *              reported through the device `status` word (Q2048_STATUS_* bits, OR-ed).
 *   - n        board side, 4 or 5 (other values return Q2048_ERR_UNSUPPORTED).  The reference
 *              hard-codes 4 (Game2048_env.py:12,41); 5 is the same algorithm on uint8[B][25]
 *              boards (unpadded) with a 125-bit state key held in `key` + `reserved`.
 */
#ifndef Q2048_H
#define Q2048_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define Q2048_ABI_VERSION 7 /* 3: flag bits outside the ABI are refused (Q2048_ERR_FLAGS), Q2048_ST_CAS_FALLBACK,
                               deterministic step sorted by a hash of (state, action)
                               4: q2048_fused_rollout_opts (row cache + statistics mirror of the fused
                               rollout), q2048_table_grow, q2048_table_alloc verifies its zero fill
                               5: growth off the caller's critical path (q2048_table_grow_begin / _poll /
                               _commit / _finish / _abort)
                               6: Q2048_FLAG_NO_NEW_ROWS (a table that has stopped taking new rows)
                               7: Q2048_FLAG_LINE_SUMMARY + q2048_table_summarise, q2048_det_rollout_cached,
                               q2048_rowcache_rebind
                               still 7, backward compatible additions: q2048_table_summarise_side and the trailing
                               field q2048_rollout_opts.line_summary (line summaries of 5x5 tables in an array beside
                               the table); q2048_fused_rollout_opts accepts both the 56-byte layout shipped before and
                               the 64-byte one, so a caller built against the earlier header runs unchanged;
                               q2048_table_merge (combine two tables on the device) arrived without a bump as well: a
                               caller detects it by its symbol; so did q2048_play_rollout (the greedy player over the
                               legal moves, one launch) and Q2048_FLAG_SYMMETRIC (one row for a board's eight mirror
                               images), detected by the symbol q2048_canonicalize; q2048_table_fold and
                               q2048_table_unfold (into and out of a folded table) likewise, each by its symbol;
                               q2048_rt_play_rollout (the greedy player on row-tuple weights) too, by its symbol;
                               the line-tuple family q2048_lt_* (rows and columns as features) by the symbol
                               q2048_lt_lookup; the afterstate value family q2048_av_* by the symbol
                               q2048_av_lookup; the 6-tuple afterstate network q2048_nt_* by the symbol
                               q2048_nt_lookup */

/* return codes */
#define Q2048_OK 0
#define Q2048_ERR_NULL (-1)        /* a required pointer is NULL */
#define Q2048_ERR_SIZE (-2)        /* negative batch / steps, bad cap_log2 */
#define Q2048_ERR_ALIGN (-3)       /* boards / aux / table not 16-byte aligned */
#define Q2048_ERR_UNSUPPORTED (-4) /* board side other than 4 or 5 */
#define Q2048_ERR_LAUNCH (-5)      /* the HIP runtime refused the launch */
#define Q2048_ERR_RANGE (-6)       /* a scalar is outside its domain (eps, lr, gamma) */
#define Q2048_ERR_FLAGS (-7)       /* flag bits outside the ABI, or flags the entry point refuses */
#define Q2048_ERR_ALLOC (-8)       /* q2048_table_alloc: memory could not be reserved / created / mapped */
#define Q2048_ERR_VERIFY (-9)      /* a table failed its self-check: a freshly mapped table did not read back as
                                      zeros, or q2048_table_grow did not find every row in the new table */
#define Q2048_ERR_BUSY (-10)       /* the table already takes part in a growth */
#define Q2048_PENDING 1            /* q2048_table_grow_poll: still working (not an error) */

/* bits of the device status word */
#define Q2048_STATUS_BAD_ACTION 1u    /* an action outside 0..3 was passed (lane left untouched) */
#define Q2048_STATUS_TILE_OVERFLOW 2u /* a tile above 2^15 does not fit the 64-bit state key */
#define Q2048_STATUS_TABLE_FULL 4u    /* an update found no slot within the probe limit (dropped) */
#define Q2048_STATUS_DEEP_ROW 8u      /* q2048_table_import placed a row deeper on its probe sequence than the learning
                                         paths look (2^10 slots; bulk moves and q2048_q_lookup take 2^14): lookup and
                                         export find it, choose / update / the rollouts read it as absent.  Only at
                                         loads above ~0.93: import into a larger table */

/* flags */
#define Q2048_FLAG_INDEPENDENT 1u /* every env owns private Q rows (key salted by its global id) */
#define Q2048_FLAG_SINGLE_ENV 2u  /* q_lookup: every board belongs to env `env_id0` (not env_id0 + i) */
#define Q2048_FLAG_TD_CAS 4u      /* TD update by a compare-and-swap loop: concurrent updates of one
                                     (s, a) serialise instead of "last writer wins" -- for up to 16
                                     attempts per update; an entry contended beyond that takes the
                                     update as a plain store, like the default mode, and the event
                                     is counted in Q2048_ST_CAS_FALLBACK: the guarantee is bounded,
                                     and the statistics say by how much.  Identical to the default
                                     whenever no two lanes share (s, a) */

#define Q2048_FLAG_ENV_DQN 8u      /* env step = the DQN path's env instead of Game2048_env.step:
                                     Deep_QLearning/environment/Game2048_nopenalty_env.py:106-138 --
                                     reward = calculate_reward2 (-10 for an invalid move while the game
                                     is not over, else the move's merge score; :122-138), done =
                                     game_over (:117-118), is_game_over evaluated on the board from
                                     BEFORE the move and, on a full board, replacing the result by its
                                     own first legal move (:68-78); the caller's write-back
                                     `env.game.board = next_state` (main_dir/mainDQL_CNN_step2.py:237)
                                     is part of the step.  No shaping state is read or written. */
#define Q2048_FLAG_RESET_SHAPING 16u /* a reset also restores previous_max and the consecutive-action
                                     state to their constructor values (Game2048_env.py:87,92-95).
                                     NOT the reference's behaviour (its reset, :187-191, keeps them:
                                     a lane ended by the >100-repeats rule ends again on its next
                                     repeat); opt-in fix of SURVEY 7.8 */
#define Q2048_FLAG_PLAY_ONLY 32u   /* fused rollout without a learner: the table is neither read nor
                                     written, every Q row reads as zeros.  With eps = 1 this is
                                     uniformly random play (input synthesis for benchmarks, the
                                     arithmetic floor of the kernel) */

#define Q2048_FLAG_NO_LEARN 64u    /* fused rollout that evaluates a trained table: rows are looked up
                                     (epsilon-greedy over the stored values), nothing is created or
                                     written.  What the `evaluate.py` the reference's README lists
                                     (README.md:52, no such file in the repository) has to do */

#define Q2048_FLAG_NO_NEW_ROWS 128u /* the table's key set is CLOSED for this call (a table that cannot
                                     grow any more "stops inserting and counts drops").  The reference's q_table is a
                                     defaultdict (Agent/main.py:16) that creates a row at every lookup of an unseen
                                     state (:38, :41, :43) and grows until the host swaps; a device table has a last
                                     capacity, and filling it to the brim makes every probe of an absent state walk
                                     hundreds of slots (12.9 ms per 2^20-board step at load 1.0 against 48 us).  With
                                     this flag
                                       - a state that has a row is read and updated exactly as without it;
                                       - a state without one reads as the zero row the defaultdict would have created
                                         (same greedy action, same bootstrap value 0), and NO row is created for it;
                                       - an update of Q[s][a] whose state has no row is dropped and counted in
                                         Q2048_ST_DROPS; Q2048_STATUS_TABLE_FULL is NOT raised (the caller asked);
                                       - VISIT ROWS: the dropped update is not lost on the env that made it.  The zero
                                         row the env read is ITS fresh row for as long as it stays in that state (the
                                         move was invalid): the update lands there, the env's next choose / update in
                                         the same state see it, and the row ends when the env moves on or its episode
                                         ends -- what the defaultdict's fresh row does within one visit (a negative
                                         reward for action 0 sends argmax on to action 1; without it a greedy env
                                         repeats an invalid action 0 until the >100-repeats rule ends the episode).
                                         The fused rollout keeps it in the lane's registers and hands it across
                                         launches through the row cache (a record without a slot); q_choose_cached /
                                         q_update_cached likewise, and q2048_det_rollout_cached keeps it in the row
                                         cache from step to step (one record format: the three paths hand visit rows to
                                         one another).  Without a row cache a visit row ends with the call -- in
                                         q2048_det_rollout, whose step keeps nothing per env, with the step.
                                     q2048_q_update / _cached, q2048_q_choose_cached, q2048_fused_rollout*,
                                     q2048_det_rollout(_cached); ignored by the entry points that neither create rows nor read
                                     the cache (q_choose, lookup, env, NO_LEARN, PLAY_ONLY).
                                     The host decides when: BatchedQLearningAgent(freeze_load=0.5) sets it on every
                                     launch once a table at its largest capacity holds that share of rows */

#define Q2048_FLAG_LINE_SUMMARY (1u << 24) /* with Q2048_FLAG_NO_NEW_ROWS: the table carries LINE SUMMARIES -- 4x4: in its
                                     slots (q2048_table_summarise ran after its last row was created); 5x5: in the array
                                     q2048_rollout_opts.line_summary names (q2048_table_summarise_side ran after the last
                                     row was created; below) -- and the fused rollout may decide a lookup from them.  A 4x4 slot has 8 spare bytes (`reserved`: the second
                                     key word of 5x5); a summary is four 16-bit fingerprints, one per slot of the
                                     128-byte line (0 = empty), the same word in all four slots.  The lookup reads the
                                     second half of the first slot of its sequence -- {q2, q3, summary}: ONE request --
                                     and knows where the sequence ends: at the first slot, in its order, that is empty
                                     (absent: done) or carries the key's fingerprint (that slot's head, one more
                                     request, settles it).  The slot-by-slot probe sends 2.35 requests per lookup on a
                                     table at load 0.5 and the step takes 47.9 us per 2^20 boards; with summaries
                                     1.25 and 34.8 us (28.7 on 64-step launches).  Same results, fewer requests.
                                     CONTRACT: the summaries describe the key set as it was when q2048_table_summarise
                                     ran.  Creating a row afterwards (any call without Q2048_FLAG_NO_NEW_ROWS, an import)
                                     makes them stale, and a stale summary HIDES rows: summarise again before the flag is
                                     passed again.  Ignored by every entry point but q2048_fused_rollout*, and there for
                                     5x5 tables WITHOUT a side array, evaluation and play-only launches (they probe slot
                                     by slot; the extra word never disturbs them: 4x4 lookups, export with key_words 1,
                                     count, import and the growth's move neither read nor write it).
                                     5x5: a slot has no spare word (`reserved` is the second key word), so the summaries
                                     live BESIDE the table: one 8-byte word per 128-byte line, 1/16 of the table's size
                                     (2 GiB beside a 32 GiB table), same format.  With Q2048_FLAG_NO_NEW_ROWS, this flag
                                     and a non-NULL q2048_rollout_opts.line_summary the fused rollout reads side[line] --
                                     one request -- per line of the sequence; an absent state is settled by it alone, a
                                     slot with the key's fingerprint costs its head and, on a first-word match, its second
                                     half.  Without the pointer the flag is ignored on 5x5; on 4x4 the pointer is ignored.
                                     (bits 8..23 belong to the measurement build's experiment switches) */

#define Q2048_FLAG_SYMMETRIC (1u << 26) /* SYMMETRY FOLDING, 4x4 only: the table holds ONE row for the eight mirror images of
                                     a board.  2048 has an eight-element symmetry group (four quarter turns, each with or
                                     without a mirror), and what the reference's reward is made of -- score, validity,
                                     max tile, game over (Game2048_env.py:136-184) -- and its spawn (uniform over the
                                     empty cells, :16-20) are invariant under it, so the true Q satisfies
                                     Q(s, a) = Q(g s, pi_g(a)): a table keyed by a canonical image needs up to 8x fewer
                                     rows for the same experience, and every row learns from all eight images.  (The only
                                     action-dependent shaping, the consecutive-action penalty, lives in `aux` and is not
                                     in the key without the flag either.)
                                       IMAGES of a board b (the [4][4] array of log2 cells), in numpy terms:
                                         g = 0..3: np.rot90(b, g), g counter-clockwise quarter turns;
                                         g = 4..7: np.rot90(np.fliplr(b), g - 4).
                                       CANONICAL IMAGE: the one whose packed 64-bit key (cell 4r + c in nibble 4r + c, as
                                         q2048_slot.key) is smallest as an unsigned integer; on a tie -- boards with a
                                         non-trivial stabiliser -- the smallest g.
                                       ACTIONS: pi_g is defined by move(image_g(b), pi_g(a)) == image_g(move(b, a)) for
                                         all b and a (a = 0 left, 1 up, 2 right, 3 down):
                                           g < 4:  pi_g(a) = (a - g) & 3        g >= 4:  pi_g(a) = (2 - a - (g - 4)) & 3
                                              a:   0 1 2 3                         a:   0 1 2 3
                                           g = 0:  0 1 2 3                      g = 4:  2 1 0 3
                                           g = 1:  3 0 1 2                      g = 5:  1 0 3 2
                                           g = 2:  2 3 0 1                      g = 6:  0 3 2 1
                                           g = 3:  1 2 3 0                      g = 7:  3 2 1 0
                                     With the flag the table is addressed by the canonical image's key (the salt of
                                     Q2048_FLAG_INDEPENDENT is applied AFTER canonicalisation) and a stored row is in the
                                     canonical frame.  Everything the caller or the policy sees is in the ENV frame,
                                     Q_env[a] = Q_canon[pi_g(a)]: the epsilon-greedy choice and its first-maximum tie order
                                     (ascending env action), the random action x1 >> 30, the player's legal mask, q_out of
                                     q2048_q_lookup, q2048_episode.q and .action.  The TD write goes to Q_canon[pi_g(a)].
                                     Where g = 0 for every board met the behaviour is that without the flag, draw for
                                     draw.  The row cache, visit rows, Q2048_FLAG_NO_NEW_ROWS and the 4x4 line summaries
                                     work unchanged (they only ever see a key); export / import / merge / growth are
                                     table-level and move canonical keys like any others.  A table is EITHER folded or
                                     plain for its whole life: the flag is a property of the table, not of a call.
                                     Taken by q2048_fused_rollout / _log / _opts, q2048_play_rollout and q2048_q_lookup
                                     (with Q2048_FLAG_PLAY_ONLY: accepted and inert); n = 5 with the flag is
                                     Q2048_ERR_UNSUPPORTED (a 125-bit compare: not built); every other entry point with
                                     a flags argument refuses it (Q2048_ERR_FLAGS).  A library that has the flag exports
                                     q2048_canonicalize (below): that symbol is how a caller detects it. */

/* per-env state, Game2048_env.__init__ (Game2048_env.py:81-95) + episode bookkeeping */
typedef struct q2048_aux {
  int32_t score;       /* env.score (:84); zeroed by reset (:190) */
  float ep_return;     /* running total_reward of Agent/main.py:84,101 */
  uint8_t prev_max;    /* log2(env.previous_max) (:87); NOT reset (:187-191) */
  uint8_t cons_action; /* env.consecutive_action (:92), 0xFF = None; NOT reset */
  uint16_t cons_count; /* env.consecutive_count (:93), saturates at 60000; NOT reset */
  uint32_t episode;    /* number of resets so far (counter of the reset draws) */
} q2048_aux;

/* one row of the Q-table: q_table[state] -> 4 floats (Agent/main.py:16) */
typedef struct q2048_slot {
  uint64_t key;      /* 4x4: 16 log2 nibbles, cell 0 in the low nibble.  5x5: bits 0..62 of the 125-bit
                        key (25 cells x 5 bits) | bit 63.  0 = empty slot */
  float q[4];        /* Q(s, a), a = 0 left, 1 up, 2 right, 3 down */
  uint64_t reserved; /* 4x4: 0 (keeps rows 32-byte aligned: a row never straddles a 64-byte line).
                        5x5: bits 63..124 of the key | bit 63, published right after `key` */
} q2048_slot;

/* one finished episode = one row of the reference's debug_log.csv (Agent/main.py:59-62,71-76:
 * Episode, Action, Q-Values, Reward, Total-Reward, Max Value), written by q2048_fused_rollout_log */
typedef struct q2048_episode {
  uint64_t env_id;    /* global env id */
  uint32_t episode;   /* index of the finished episode within that env ("Episode") */
  uint8_t action;     /* last action ("Action") */
  uint8_t max_log2;   /* log2 of the max tile of the final board ("Max Value" = 2^max_log2) */
  uint16_t steps_lo;  /* low 16 bits of the global step counter at which the episode ended */
  float reward;       /* last reward ("Reward") */
  float total_return; /* sum of the episode's rewards ("Total-Reward") */
  int32_t score;      /* env.score at the end */
  float q[4];         /* post-update Q row of the last state ("Q-Values", main.py:96 aliases the row) */
  uint32_t reserved;
} q2048_episode;

/* indices of the statistics vectors (device int64[Q2048_NSTAT_I], double[Q2048_NSTAT_F]);
 * kernels ADD to them, the caller zeroes them */
enum {
  Q2048_ST_STEPS = 0,    /* env steps executed */
  Q2048_ST_EPISODES = 1, /* episodes finished */
  Q2048_ST_VALID = 2,    /* board-changing moves */
  Q2048_ST_SCORE = 3,    /* sum of env.score over finished episodes */
  Q2048_ST_INSERTS = 4,  /* Q rows created */
  Q2048_ST_DROPS = 5,    /* updates dropped: no slot within the probe limit, or (Q2048_FLAG_NO_NEW_ROWS) no row */
  Q2048_ST_EXPLORE = 6,  /* epsilon branch taken */
  Q2048_ST_CAS_RETRY = 7,/* TD compare-and-swap retries (same (s,a) updated concurrently) */
  Q2048_ST_HIST0 = 8,    /* max-tile histogram of finished episodes, log2 0..22 (saturating) */
  Q2048_ST_CAS_FALLBACK = 31, /* Q2048_FLAG_TD_CAS updates that lost 16 races in a row and were
                                 written as a plain store instead */
  Q2048_NSTAT_I = 32
};
enum { Q2048_SF_RETURN = 0, Q2048_SF_RETURN_SQ = 1, Q2048_SF_REWARD = 2, Q2048_NSTAT_F = 4 };

int q2048_abi_version(void);

/* Diagnostic, host-synchronous: lanes of the current device that ever gave up waiting for the
 * second key word of a 5x5 row under creation (the wait is bounded so that a protocol error can
 * never hang the device).  Expected value: 0, always; the tests assert it. */
int q2048_claim_timeouts(uint64_t *count_host);
const char *q2048_strerror(int code);
size_t q2048_sizeof_aux(void);  /* 16 */
size_t q2048_sizeof_slot(void); /* 32 */

/* Game2048_env() constructor for B envs (Game2048_env.py:81-95 -> Game2048.__init__ :11-14):
 * empty board + two spawns from the reset draws of episode 0, aux = initial values. */
int q2048_env_init(uint8_t *boards, q2048_aux *aux, int64_t B, int n, uint64_t seed,
                   uint64_t env_id0, void *stream);

/* Game2048_env.reset() (Game2048_env.py:187-191) for the lanes with mask[i] != 0 (all lanes
 * when mask == NULL): new board with two spawns, score = 0; previous_max and the
 * consecutive-action state persist, as in the reference. */
int q2048_env_reset(uint8_t *boards, q2048_aux *aux, const uint8_t *mask, int64_t B, int n,
                    uint64_t seed, uint64_t env_id0, void *stream);

/* q2048_env_reset with flags (Q2048_FLAG_RESET_SHAPING; other bits ignored). */
int q2048_env_reset_ex(uint8_t *boards, q2048_aux *aux, const uint8_t *mask, int64_t B, int n,
                       uint64_t seed, uint64_t env_id0, uint32_t flags, void *stream);

/* Game2048_env.step(action) (Game2048_env.py:97-129) for B envs: move (:51-63), game-over
 * probe (:65-75), shaped reward (:136-184, :197-205), stall rule (:110-127).
 * Outputs per lane: reward (float32 of the reference's float), done, max tile as log2
 * (reference `info` = 2^max_log2).  An action outside 0..3 leaves its lane untouched and
 * sets Q2048_STATUS_BAD_ACTION (the reference would silently mis-rotate, :56-60). */
int q2048_env_step(uint8_t *boards, q2048_aux *aux, const uint8_t *actions, int64_t B, int n,
                   uint64_t seed, uint64_t env_id0, uint32_t ctr, float *reward, uint8_t *done,
                   uint8_t *max_log2, uint32_t *status, void *stream);

/* q2048_env_step with the two spawn decisions' raw draws given per lane instead of derived from
 * (seed, id, ctr): draw_pos replaces np.random.randint(0, n_empty) (Game2048_env.py:19),
 * draw_val replaces np.random.random() < 0.9 (:20).  Draw injection is how parity with the
 * reference is pinned (tests/golden); training uses q2048_env_step. */
int q2048_env_step_draws(uint8_t *boards, q2048_aux *aux, const uint8_t *actions,
                         const uint32_t *draw_pos, const uint32_t *draw_val, int64_t B, int n,
                         float *reward, uint8_t *done, uint8_t *max_log2, uint32_t *status,
                         void *stream);

/* q2048_env_step with an env profile: flags = Q2048_FLAG_ENV_DQN selects the DQN path's step
 * (Game2048_nopenalty_env.py:106-138, see the flag); 0 = q2048_env_step.  draws4 = NULL: draws
 * derived from (seed, id, ctr) -- the chosen move's spawn from words 2, 3 of stream 0 as always,
 * the spawn inside is_game_over's move from words 0, 1 of stream 2.  draws4 = uint32[B][4]:
 * injected draws {pos, val, over_pos, over_val} per env (parity with the reference; seed /
 * env_id0 / ctr are then unused). */
int q2048_env_step_ex(uint8_t *boards, q2048_aux *aux, const uint8_t *actions, int64_t B, int n,
                      uint64_t seed, uint64_t env_id0, uint32_t ctr, uint32_t flags,
                      const uint32_t *draws4, float *reward, uint8_t *done, uint8_t *max_log2,
                      uint32_t *status, void *stream);

/* q2048_env_step_ex (draws derived from (seed, id, ctr)) reading boards_in and writing boards_out:
 * the same buffer (in place), or two buffers that do not overlap -- then the state before the step
 * stays intact for update_q_value(state, ...) and the batched loop of Agent/main.py:92-100 needs no
 * board copy (the host side ping-pongs two buffers).  A lane with a rejected action copies its
 * board unchanged.  max_tile (may be NULL): int32[B], the reference's `info` -- the raw max tile
 * (Game2048_env.py:100,129) -- written next to its log2. */
int q2048_env_step_to(const uint8_t *boards_in, uint8_t *boards_out, q2048_aux *aux,
                      const uint8_t *actions, int64_t B, int n, uint64_t seed, uint64_t env_id0,
                      uint32_t ctr, uint32_t flags, float *reward, uint8_t *done, uint8_t *max_log2,
                      int32_t *max_tile, uint32_t *status, void *stream);

/* QLearningAgent.choose_action(state) (Agent/main.py:34-38) for B states: epsilon test and
 * random action from the step draws, else first-maximum argmax of the row (zeros if absent;
 * a lookup never inserts -- value-equivalent to the defaultdict). */
int q2048_q_choose(const q2048_slot *table, int cap_log2, const uint8_t *boards, int64_t B,
                   int n, double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr,
                   uint32_t flags, uint8_t *actions, uint32_t *status, void *stream);

/* q2048_q_choose with injected draws: draw_eps replaces random.random() (Agent/main.py:35),
 * draw_act replaces random.randint(0, 3) (:36). */
int q2048_q_choose_draws(const q2048_slot *table, int cap_log2, const uint8_t *boards,
                         const uint32_t *draw_eps, const uint32_t *draw_act, int64_t B, int n,
                         double eps, uint64_t env_id0, uint32_t flags, uint8_t *actions,
                         uint32_t *status, void *stream);

/* QLearningAgent.update_q_value(state, action, reward, next_state, done)
 * (Agent/main.py:40-43) for B transitions.  Rows for next_state and state are created when
 * absent, as the reference's defaultdict does (:41-43).  Q[s][a] is written with one 4-byte
 * store: lanes that update the same (s, a) concurrently race and the last writer wins
 * (Q2048_FLAG_TD_CAS serialises them with a compare-and-swap loop instead).  With one lane, or
 * lanes on disjoint states, this is exactly the reference's sequential update. */
int q2048_q_update(q2048_slot *table, int cap_log2, const uint8_t *boards_s,
                   const uint8_t *actions, const float *reward, const uint8_t *boards_s2,
                   const uint8_t *done, int64_t B, int n, double lr, double gamma,
                   uint64_t env_id0, uint32_t flags, int64_t *stats_i, uint32_t *status,
                   void *stream);

/* Row cache of the 4-call API: q2048_q_update / q2048_q_choose with a caller-owned device buffer of
 * B records of q2048_sizeof_rowcache(n) bytes (32 for n = 4, 48 for n = 5; 16-byte aligned;
 * zero-filled = empty; NULL = the plain entry points).  q_update leaves in record i the row env i
 * read as next_state -- key, slot, the four values, with its own write folded in when the move was
 * invalid -- and the next q_choose / q_update of the same env use it instead of probing when the
 * board they are given has that key: in the loop of Agent/main.py:92-100 `state` IS the previous
 * `next_state` unless an episode began, so an update costs one scattered row read instead of two
 * and a greedy choose none.  This is what the fused rollout carries in registers, handed over
 * through HBM as a stream; like it, a cached row does not see what OTHER envs wrote to it since.
 * Any calling pattern is correct: a record is used only when its key is the key of the board passed in AND it
 * was left by a call on this very table.  The contract for that second half: THE CALLER ZERO-FILLS THE CACHE whenever
 * the table behind it changes -- a growth's commit (slots change), another table, a table rewritten in place
 * (zero-filled, imported into, updated through an entry point without the cache).  As a safety net every record also
 * carries a 24-bit tag of the table's address and capacity, so that records of another table miss instead of steering
 * writes through stale slot indices -- with probability 1 - 2^-24 per pair of tables: a net, not the contract. */
size_t q2048_sizeof_rowcache(int n);
/* A cache's VISIT ROWS (Q2048_FLAG_NO_NEW_ROWS) follow their table's rows into another allocation -- a checkpoint of
 * a learner with a closed key set, restored: the host saves the cache's bytes beside the table's rows, the old
 * table's address and capacity (two numbers; `from_table` is never dereferenced), restores the rows into `to_table`
 * (any capacity that holds them) and calls this on the restored bytes.  Every record without a slot that a call on
 * `from_table` left becomes one of `to_table`; every other record is emptied (a slot index of the old allocation
 * means nothing in the new one).  The resumed run then equals the uninterrupted one step for step; without it the
 * envs that were in a state without a row at the checkpoint start that visit again from the zero row.  The two
 * tables must hold the SAME KEY SET (a visit row stands in for a row that does not exist). */
int q2048_rowcache_rebind(void *row_cache, int64_t B, int n, const q2048_slot *from_table, int from_cap_log2,
                          const q2048_slot *to_table, int to_cap_log2, void *stream);
int q2048_q_choose_cached(const q2048_slot *table, int cap_log2, const uint8_t *boards, int64_t B,
                          int n, double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr,
                          uint32_t flags, const void *row_cache, uint8_t *actions,
                          uint32_t *status, void *stream);
int q2048_q_update_cached(q2048_slot *table, int cap_log2, const uint8_t *boards_s,
                          const uint8_t *actions, const float *reward, const uint8_t *boards_s2,
                          const uint8_t *done, int64_t B, int n, double lr, double gamma,
                          uint64_t env_id0, uint32_t flags, void *row_cache, int64_t *stats_i,
                          uint32_t *status, void *stream);

/* agent.q_table[state] (Agent/main.py:16,96) for B states: q_out[B][4] (zeros if absent),
 * found[B] (may be NULL). */
int q2048_q_lookup(const q2048_slot *table, int cap_log2, const uint8_t *boards, int64_t B,
                   int n, uint64_t env_id0, uint32_t flags, float *q_out, uint8_t *found,
                   uint32_t *status, void *stream);

/* The loop body of Agent/main.py:91-101 + the reset of :81, `steps` times for B envs in ONE
 * launch: choose -> step -> update -> accumulate -> (on done) statistics and reset.  Boards,
 * aux and the Q row of the current state stay in registers between steps.  Step t uses the
 * draws of counter ctr0 + t.  Bit-identical to calling q_choose / env_step / q_update /
 * env_reset(done) `steps` times whenever no two lanes share a state.
 * flags: Q2048_FLAG_INDEPENDENT, _TD_CAS, _ENV_DQN, _RESET_SHAPING, _PLAY_ONLY, _NO_LEARN, _NO_NEW_ROWS; any
 * bit outside the Q2048_FLAG_* set is Q2048_ERR_FLAGS (all entry points). */
int q2048_fused_rollout(uint8_t *boards, q2048_aux *aux, q2048_slot *table, int cap_log2,
                        int64_t B, int n, int64_t steps, double eps, double lr, double gamma,
                        uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                        int64_t *stats_i, double *stats_f, uint32_t *status, void *stream);

/* q2048_fused_rollout that also appends one q2048_episode record per finished episode to
 * log[0 .. log_capacity) (log_count is a device uint64 cursor the caller zeroes; records beyond
 * the capacity are counted but not written).  This is the device form of log_debug_info
 * (Agent/main.py:59-62, called at :103-105). */
int q2048_fused_rollout_log(uint8_t *boards, q2048_aux *aux, q2048_slot *table, int cap_log2,
                            int64_t B, int n, int64_t steps, double eps, double lr, double gamma,
                            uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                            int64_t *stats_i, double *stats_f, uint32_t *status,
                            q2048_episode *log, int64_t log_capacity, uint64_t *log_count,
                            void *stream);

/* q2048_fused_rollout with optional extras, all caller-owned, any of them NULL (opts == NULL is
 * q2048_fused_rollout itself).  The launch boundary cuts the loop of Agent/main.py:91-101 between two
 * iterations; the extras are what makes a cut cheap:
 *   log, log_capacity, log_count   as q2048_fused_rollout_log.
 *   row_cache   the row cache of the 4-call API (above: q2048_sizeof_rowcache(n) bytes per env, 16-byte
 *               aligned, zero-filled = empty), shared with it.  A launch ENDS by leaving in record i the row
 *               env i carries in registers -- key, the four values, slot -- and STARTS from that record when
 *               its key is the key of the board it is given (a coalesced 32-byte read) instead of probing
 *               the table (a scattered 128-byte request per lane: 21.5 us of every launch at 2^20 boards).
 *               K steps in launches of S with the cache are the K-step launch: a row is carried across the
 *               cut exactly as across a step.  Any calling pattern is correct (a record is used only on a
 *               key match); like a row carried in registers, a record does not see what OTHER envs wrote to
 *               its row since.  Q2048_FLAG_PLAY_ONLY launches neither read nor write it.
 *   stats_mirror, mirror_ticket   stats_mirror: (Q2048_NSTAT_I + Q2048_NSTAT_F + 1) 8-byte words the HOST
 *               can read while the device writes them -- pinned host memory mapped into the device's
 *               address space (hipHostMalloc; any 8-byte aligned pointer the device can store to works).
 *               The last block of the launch to finish copies stats_i then stats_f (both required then), as
 *               they stand after the whole launch's additions, into words 0..35 and writes the number of
 *               mirrored launches so far into word Q2048_MIRROR_SEQ: a caller that waits for the launch
 *               anyway (hipStreamSynchronize) reads its statistics from host memory with no copy queued
 *               behind the kernel.  mirror_ticket: device uint32[2], zero before its first use, private to
 *               one stream of launches (two launches that share it must not overlap).
 *   line_summary   the line summaries of a 5x5 table with a closed key set (Q2048_FLAG_LINE_SUMMARY above).
 * `size` = sizeof(q2048_rollout_opts) as the caller was built: 64, or the 56 bytes of the layout without
 * `line_summary`; a caller built against any other layout is refused (Q2048_ERR_SIZE). */
#define Q2048_MIRROR_SEQ 36 /* = Q2048_NSTAT_I + Q2048_NSTAT_F */
#define Q2048_MIRROR_WORDS 37
typedef struct q2048_rollout_opts {
  uint32_t size;
  uint32_t reserved;
  q2048_episode *log;
  int64_t log_capacity;
  uint64_t *log_count;
  void *row_cache;
  void *stats_mirror;
  uint32_t *mirror_ticket;
  const uint64_t *line_summary; /* 5x5, Q2048_FLAG_NO_NEW_ROWS | Q2048_FLAG_LINE_SUMMARY: the side array
                                   q2048_table_summarise_side wrote for THIS table and key set (2^(cap_log2-2) words,
                                   8-byte aligned, else Q2048_ERR_ALIGN); NULL = none (slot-by-slot probe).  Trailing field,
                                   added after the 56-byte layout: `size` = 56 is accepted and means NULL */
} q2048_rollout_opts;
int q2048_fused_rollout_opts(uint8_t *boards, q2048_aux *aux, q2048_slot *table, int cap_log2,
                             int64_t B, int n, int64_t steps, double eps, double lr, double gamma,
                             uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                             int64_t *stats_i, double *stats_f, uint32_t *status,
                             const q2048_rollout_opts *opts, void *stream);

/* The GREEDY PLAYER: what a trained table is worth when only moves that change the board are made -- `steps` steps
 * for B envs in ONE launch, the table only read.  It replaces the loop q_lookup / legal_moves / env_step /
 * env_reset(done) (evaluate.py --policy legal): the legal-move mask is the trial-move loop of
 * Deep_QLearning/main_dir/mainDQL_CNN_step2.py:168-174, the choice the argmax of Agent/main.py:34-38 restricted to it.
 * One step of one env (lane i = global env env_id0 + i, counter ctr0 + t):
 *   row     the state's row exactly as q2048_q_lookup reads it (same probe and probe limit: rows beyond the learning
 *           paths' limit are found; Q2048_FLAG_INDEPENDENT salts the key with the env's id; an absent state reads as
 *           zeros; `reserved` is never interpreted, so a 4x4 table that carries line summaries plays the same);
 *   mask    bit a set iff action a would change the board (q2048_legal_moves);
 *   action  the first maximum of the row over the legal moves: ascending action order, strict > (np.argmax of the
 *           masked row; +0 and -0 compare equal).  No legal move: action 0;
 *   explore DRAW CONTRACT of the player: the step's one Philox call (stream 0 of (seed, env id, ctr0 + t), the call
 *           q2048_env_step makes) gives x0..x3.  The env explores iff x0 < ceil(eps * 2^32) (eps >= 1: always, eps = 0:
 *           never -- the integer form of x0 / 2^32 < eps) AND it has a legal move; its move is then the k-th legal one
 *           in ascending order, k = (x1 * n_legal) >> 32.  With no legal move the action stays 0 and the step is not
 *           counted as explored.  (q2048_q_choose draws its random action from all four: x1 >> 30.)
 *   step    q2048_env_step's step with x2, x3 of the same call (Q2048_FLAG_ENV_DQN: the DQN path's env, its
 *           is_game_over spawn from words 0, 1 of stream 2) -- the draws q2048_env_step uses at counter ctr0 + t; on
 *           done the episode statistics and the reset of q2048_fused_rollout.
 * Written: boards, aux, the statistics -- steps, valid, explore, episodes, the score / return sums, the max-tile
 * histogram and the reward sum, ADDED to stats_i / stats_f (either may be NULL; inserts and drops stay 0) -- and
 * Q2048_STATUS_TILE_OVERFLOW.  Never the table, no row cache, no other status bit: the result is a function of
 * (table, boards, aux, seed, env ids, counter) at any B.
 * flags: Q2048_FLAG_INDEPENDENT, _ENV_DQN, _RESET_SHAPING; any other Q2048_FLAG_* bit, and any bit outside the ABI, is
 * Q2048_ERR_FLAGS.  eps outside [0, 1] is Q2048_ERR_RANGE.  B == 0 or steps == 0: nothing happens, Q2048_OK.  Argument
 * errors in the order of q2048_fused_rollout: n, B, flags, table (NULL, cap_log2, alignment), boards / aux / status
 * NULL, their alignment, steps, eps. */
int q2048_play_rollout(uint8_t *boards, q2048_aux *aux, const q2048_slot *table, int cap_log2, int64_t B, int n,
                       int64_t steps, double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                       int64_t *stats_i, double *stats_f, uint32_t *status, void *stream);

/* Deterministic mode: reproducible shared-table training at any B (the default rollout is
 * lock-free and depends on scheduling wherever lanes share a state).  Per step:
 *   phase 1  every env chooses on, steps, and reads max Q(s') from the table as it is at the
 *            START of the step (phase 1 writes no Q value; it creates the rows of s and s' like
 *            update_q_value does, Agent/main.py:41-43) and emits its update: (row slot, action)
 *            and the TD target reward + gamma * max Q(s') * (1 - done) (:42);
 *   sort     the updates are sorted on the device, stably, by a 16-bit hash of (state, action):
 *            the updates of a group end up in one short run, in env order;
 *   phase 2  every group applies Q[s][a] += lr * (target - Q[s][a]) (:43) update by update in env
 *            order, in the reference's double arithmetic (no fused multiply-add), and rounds to
 *            float32 once per group and step.
 * The result equals the reference agent fed the step's transitions in env order against the
 * step-start table with its rows held as float32, for any B, and is a function of the inputs
 * alone: the sort key depends on the state and the action, never on which slot a racing insert
 * won, and every group is folded by the same sequence of operations whatever its size.  `steps`
 * steps per call, draws of counter ctr0 + t.  flags: Q2048_FLAG_INDEPENDENT, _ENV_DQN,
 * _RESET_SHAPING, _NO_NEW_ROWS; _TD_CAS is ignored; _NO_LEARN and _PLAY_ONLY are refused (Q2048_ERR_FLAGS: there
 * is no evaluation form of this step, and learning anyway would be the wrong answer).
 * `workspace`: caller-owned device scratch of q2048_det_workspace_bytes(B, cap_log2) bytes
 * (about 36 bytes per env; host arithmetic, needs no device), 256-byte aligned (B < 2^31).  It
 * holds no state between calls. */
int64_t q2048_det_workspace_bytes(int64_t B, int cap_log2);
int q2048_det_rollout(uint8_t *boards, q2048_aux *aux, q2048_slot *table, int cap_log2, int64_t B,
                      int n, int64_t steps, double eps, double lr, double gamma, uint64_t seed,
                      uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t *stats_i,
                      double *stats_f, uint32_t *status, void *workspace, int64_t workspace_bytes,
                      void *stream);
/* ... with the envs' row cache (B records of q2048_sizeof_rowcache(n) bytes, 16-byte aligned, the one the fused
 * rollout and the _cached calls take; NULL = q2048_det_rollout).  Used with Q2048_FLAG_NO_NEW_ROWS only, for VISIT
 * ROWS: an env in a state without a row reads its visit row in phase 1, and while it stays there its update --
 * dropped from the table and counted as before -- lands in that row (float32, the fused rollout's arithmetic; it is
 * one env's, so it needs no ordering and the result stays a function of the inputs alone).  Every record the call
 * touches is left either a visit row or empty: records of table rows left by a fused launch are cleared, never
 * used.  Without the flag the cache is neither read nor written. */
int q2048_det_rollout_cached(uint8_t *boards, q2048_aux *aux, q2048_slot *table, int cap_log2, int64_t B,
                             int n, int64_t steps, double eps, double lr, double gamma, uint64_t seed,
                             uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t *stats_i,
                             double *stats_f, uint32_t *status, void *workspace, int64_t workspace_bytes,
                             void *row_cache, void *stream);

/* Table allocation from small physical chunks -- the ONLY entry points that allocate (everything
 * else works on caller-owned memory, however it was obtained; a table from hipMalloc / a framework
 * allocator is as valid).  Why it exists: the rate at which this memory system takes scattered
 * 4-byte stores and atomics depends on how the table's memory was obtained.  A table mapped from
 * 2 MiB physical chunks (HIP virtual-memory API: hipMemCreate + hipMemMap into one reserved range)
 * takes them 15-20 % faster than a hipMalloc of the same 8-32 GiB (load + compare-and-swap + store
 * per lane-step: 46.2 against 55.4 us per 2^20 on an 8 GiB table, 51.2 with 64 MiB chunks;
 * profiles/r03_requests/vmm_*_8GiB.txt; loads do not care) -- as fast as a table that spans 128 GiB.
 * (Round 4, six fresh allocations per chunk size: 2, 8, 32 and 64 MiB chunks overlap completely,
 * profiles/r04_requests/chunk_size_six_draws.txt -- the effect is mapped memory against hipMalloc and
 * which allocation one got, not the chunk size.)
 *
 * q2048_table_alloc reserves, creates, maps and zero-fills 2^cap_log2 slots (chunk_bytes = 0: 2 MiB;
 * else a power of two that is a multiple of the allocation granularity) on the current device, and VERIFIES the zero fill
 * with one streaming count of the table before it returns (Q2048_ERR_VERIFY otherwise: a slot that
 * wrongly looks occupied is how rows would get lost silently).  Host-synchronous.
 *
 * A table that grows -- the reference's defaultdict (Agent/main.py:16) has no capacity:
 * q2048_table_reserve maps a table of 2^cap_log2 slots that may grow up to 2^max_cap_log2 (and allocates the
 * family's 64 bytes of scratch and its private stream: nothing below calls hipMalloc / hipFree).  Growing =
 * mapping the table of capacity 2^new_cap_log2 (cap_log2 < new_cap_log2 <= max_cap_log2) onto fresh chunks in
 * an address range of its own, moving every row over in one streaming pass (the rows keep their values; their
 * slots change: zero-fill any row cache), and releasing the old table.  The table's ADDRESS changes.
 *
 * Off the caller's critical path (the reference's dict grows without stopping the loop, Agent/main.py:16,91-101):
 *   q2048_table_grow_begin(table, cap_log2, new_cap_log2, &g)   returns at once; ONE host thread of the library
 *       (started by the first call, joined at exit) reserves, creates, maps, zero-fills and verifies the new table
 *       on the family's own stream while the caller keeps launching rollouts on the old one: 31 ms for 32 GiB,
 *       119 ms for 128 GiB next to a stream of launches that slow by 16 % meanwhile
 *       (profiles/r05_vmm_cost_small_chunks.txt).
 *   q2048_table_grow_poll(g)      Q2048_OK: the next call (commit, or finish after a commit) will not block;
 *       Q2048_PENDING: it would; < 0: the preparation failed (commit returns the same code and ends the growth).
 *   q2048_table_grow_wait(g, &ms)   blocks until the preparation is over (a caller that prefers to wait before its
 *       clock starts rather than at the commit) and returns its outcome; ms (host double, may be NULL) = what the
 *       host thread spent on it.
 *   q2048_table_grow_commit(g, key_words, flags, &bigger, stream)   waits for the preparation if need be, then
 *       enqueues the move (k_table_rehash, 18 G rows/s) on `stream`, behind whatever the caller queued on the old
 *       table, and returns the new table WITHOUT waiting for it: every launch queued on `stream` from here on
 *       takes *bigger.  flags: Q2048_GROW_VERIFY_COUNT also counts the new table's rows behind the move (one more
 *       streaming pass, 21 ms per 128 GiB).  Errors: Q2048_ERR_NULL / _SIZE / _FLAGS (arguments) and Q2048_ERR_BUSY
 *       (another growth of the family is committed and not yet finished, or another thread is committing this very
 *       growth) change nothing -- g is STILL VALID: retry after the other growth's finish, or q2048_table_grow_abort(g).
 *       Any other error (the preparation failed: its code; Q2048_ERR_LAUNCH) ends the growth: the old table is intact
 *       and still the caller's, the prepared table has been released, g is gone.
 *   q2048_table_grow_finish(g, &rows)   waits for the move, checks it -- every occupied slot of the old table found
 *       its place (and, with VERIFY_COUNT, the new table holds exactly that many rows): Q2048_ERR_VERIFY otherwise,
 *       both tables then stay live and g is gone; Q2048_ERR_LAUNCH when the wait itself failed: nothing is known
 *       about the move, g stays valid (retry, or free the tables: q2048_table_free resolves the growth) -- and
 *       RETIRES the old table: it is the library's from here on (do not free or
 *       touch it) and its memory is kept until a mapping on the device finds no room, the family's last live table
 *       is freed, or q2048_table_trim(live table) asks for it -- because memory a process releases is wiped by the
 *       driver at ~40 GB/s before it is handed out again, and the next mapping would wait for that: hipMemCreate of
 *       128 GiB takes 30 ms on memory that has been free for a while and 3-4 s right after 128 GiB were released,
 *       by this or by the previous process (profiles/r05_vmm_wipe.txt).  rows (host int64, may be NULL) = rows
 *       moved = the occupied slots of the old table: compare it with the rows the kernels reported
 *       (Q2048_ST_INSERTS) and the old table is verified end to end.
 *   q2048_table_grow_abort(g)     before the commit: the prepared table is released, the old one untouched.
 * One growth per table at a time (Q2048_ERR_BUSY); the next growth of the NEW table may begin right after the
 * commit, its commit only after the previous finish.  q2048_table_grow(...) is begin + commit(VERIFY_COUNT) +
 * finish + the release of the old table in one host-synchronous call.  While both tables exist the device holds both.
 *
 * Chunk sizes: a table of a family that can grow is cut into as few chunks as 32 MiB allows (2 MiB up to 2 GiB,
 * bytes / 1024 up to 32 GiB, 32 MiB beyond: 4096 chunks for 128 GiB).  hipMemMap / hipMemUnmap / hipMemSetAccess
 * cost 5-16 us per chunk (more, the more chunks a process holds: 2 MiB chunks for 128 GiB took 13.8 s,
 * profiles/r04_growth_phases_2MiB_chunks.txt); what hipMemCreate costs depends on the state of the device's free
 * memory, not on the chunk: 4-30 us per chunk on memory that has been free for a while, seconds per table (at any
 * chunk size from 8 MiB to 1 GiB) when the driver hands out memory that was released moments before, by this or
 * by the previous process, and is still being wiped (profiles/r05_vmm_cost_by_chunk.txt,
 * r05_vmm_cost_small_chunks.txt, r05_vmm_wipe.txt: 3.2-3.9 s right after, 30 ms twelve seconds later) -- which is
 * what round 4's 1.9 s for the step to 128 GiB was.  q2048_table_alloc keeps the chunk size it is asked for.
 * The caller decides when to grow: between launches, when rows created / capacity passes its load limit (the
 * rollout's step slows from 46.7 to 66.3 us as the load goes from 0.12 to 0.54, profiles/r03_load_curve.jsonl).
 *
 * q2048_table_free unmaps a table's chunks and releases their physical memory (it synchronises the
 * table's device first, whatever the calling thread's current device is; a growth the table takes part in is
 * resolved first: aborted if uncommitted, finished if committed).  THE ADDRESS RANGE STAYS
 * RESERVED until the process ends and no part of it is ever mapped a second time -- a range that is
 * freed, reserved again and mapped onto new chunks serves stale translations on ROCm 7.2: tables on a re-used
 * range lose 0.01-1.3 % of the rows written to them, with every HIP call returning success.  Library-free
 * reproducer: tools/va_reuse_repro.hip (152 lines of HIP; profiles/r05_va_reuse_repro.txt: 0 of 8 tables lose
 * rows on fresh ranges, 4 of 8 on a re-used one, 1 of 8 with a device synchronize after the free).  A process
 * therefore accumulates reserved address space -- 2^-12 of its 47-bit space per 32 GiB table -- not memory.
 * For the same reason tables are reserved in a PRIVATE REGION of the address space (16 TiB upward, one range per table
 * from a process-wide cursor; the runtime's own allocations grow down from the top): after a large hipFree the next
 * un-hinted hipMemAddressReserve returns exactly the freed address (tools/va_hint_probe.hip), so a table reserved the
 * ordinary way could sit on a range some other allocator had mapped before.  And room is asked for (hipMemGetInfo)
 * before a single chunk is created: Q2048_ERR_ALLOC comes back at once when the device cannot hold the table, because
 * mapping chunk by chunk until hipMemCreate fails left this stack in a state in which the process's next large mapping
 * faulted the GPU (profiles/r06_va_reuse_fault.txt).
 * All of these are thread-safe. */
#define Q2048_GROW_VERIFY_COUNT 1u
typedef struct q2048_growth q2048_growth; /* opaque: a growth between begin and finish / abort */
int q2048_table_alloc(int cap_log2, size_t chunk_bytes, q2048_slot **table_out);
int q2048_table_reserve(int cap_log2, int max_cap_log2, size_t chunk_bytes, q2048_slot **table_out);
int q2048_table_grow_begin(q2048_slot *table, int cap_log2, int new_cap_log2, q2048_growth **growth_out);
int q2048_table_grow_poll(q2048_growth *growth);
int q2048_table_grow_wait(q2048_growth *growth, double *prepare_ms);
int q2048_table_grow_commit(q2048_growth *growth, int key_words, uint32_t flags, q2048_slot **table_out,
                            void *stream);
int q2048_table_grow_finish(q2048_growth *growth, int64_t *rows_moved);
int q2048_table_grow_abort(q2048_growth *growth);
int q2048_table_grow(q2048_slot *table, int cap_log2, int new_cap_log2, int key_words,
                     q2048_slot **table_out, int64_t *rows_moved, void *stream);
int q2048_table_trim(q2048_slot *table); /* releases the retired predecessors of this table's family now */
int q2048_table_free(q2048_slot *table);

/* Placement probe (no reference counterpart): `lanes` lanes each issue `steps` scattered
 * device-scope atomic ORs of 0 on key words of the table -- the write-side request pattern of
 * the rollout, leaving every byte of the table as it was, so it may run on a live table.  The
 * caller times it to choose among candidate allocations (the scattered write / atomic rate
 * depends on where in device memory a table lies; reads do not). */
int q2048_table_probe(q2048_slot *table, int cap_log2, int64_t lanes, int steps, uint64_t seed,
                      void *stream);

/* Writes the LINE SUMMARIES of a 4x4 table whose key set is closed (Q2048_FLAG_LINE_SUMMARY above): one streaming pass
 * over the table (reads every key, writes every slot's `reserved` word; 19.7 ms per 32 GiB), stream-ordered.  Run it
 * after the last row was created and before the first launch that carries the flag; run it again if rows were created
 * since.  MUST NOT be called on a 5x5 table: its `reserved` words are the second key words, and this pass overwrites
 * them (every row of the table is lost, silently).  For 5x5 use q2048_table_summarise_side. */
int q2048_table_summarise(q2048_slot *table, int cap_log2, void *stream);

/* The LINE SUMMARIES of a table in caller-owned memory BESIDE it -- the form for 5x5 tables (key_words = 2), whose slots
 * have no spare word: one streaming pass that reads the table and writes 2^(cap_log2-2) words to `summary`; the table is
 * never written.  Word l describes line l (slots 4l .. 4l+3): bits 16r .. 16r+15 are 0 when slot 4l+r is empty
 * (key == 0), else ((hash >> 48) & 0xffff) | 1 with `hash` the table's own hash of the slot's key (key_words 1:
 * mix64(key); 2: mix64(key ^ reserved * 0x9E3779B97F4A7C15)) -- the format of the in-slot summaries, so with
 * key_words = 1 the words equal what q2048_table_summarise puts into the slots.  Memory: 8 bytes per 128-byte line,
 * 1/16 of the table (2 GiB beside 32 GiB, 8 GiB beside 2^32 slots).  Stream-ordered.
 * Same contract as the in-slot summaries: the words describe the key set as it was when the pass ran.  Run it when no
 * call that creates rows is in flight (queued behind the last one on the same stream), and again after anything that
 * may have created rows, before q2048_rollout_opts.line_summary is passed with Q2048_FLAG_LINE_SUMMARY again.
 * Errors: table or summary NULL -> Q2048_ERR_NULL; key_words not 1 or 2 -> Q2048_ERR_SIZE; summary not 8-byte aligned
 * -> Q2048_ERR_ALIGN; then cap_log2 / the table's alignment as everywhere. */
int q2048_table_summarise_side(const q2048_slot *table, int cap_log2, int key_words, uint64_t *summary, void *stream);

/* len(agent.q_table): adds the number of occupied slots to *count (device int64). */
int q2048_table_count(const q2048_slot *table, int cap_log2, int64_t *count, void *stream);

/* Export occupied rows (for conversion to the reference's dict{state -> 4 floats},
 * Agent/main.py:16): writes (key, q[4]) pairs in unspecified order and adds the number of occupied
 * slots to *count.
 * *count IS THE WRITE CURSOR of the export, as log_count is for the episode log: the records of this call
 * go to indices [count0, count0 + occupied) of keys_out / q_out, count0 being the value of *count when the
 * call starts, and max_rows is the capacity of the buffers -- an index bound, not a number of rows of this
 * call: a record whose index is >= max_rows is counted, not written (which rows those are is unspecified).
 * A caller that wants the rows from index 0 zeroes *count first; tables exported one after the other into
 * the same buffers with the same cursor end up side by side.  Nothing outside [count0, max_rows) is touched.
 * key_words = 1 (4x4: keys_out[max_rows]; the `reserved` words -- 0 or line summaries -- are not exported)
 * or 2 (5x5: keys_out[max_rows][2] = key, reserved).  keys_out and q_out are both NULL (count only) or
 * both given; q_out 16-byte aligned.  The table is only read. */
int q2048_table_export(const q2048_slot *table, int cap_log2, uint64_t *keys_out, float *q_out,
                       int64_t max_rows, int key_words, int64_t *count, void *stream);

/* Legal-move mask: bit a of mask_out[i] is set iff action a would change board i -- the trial-move
 * loop of Deep_QLearning/main_dir/mainDQL_CNN_step2.py:168-174 (`env.game.move(action,
 * trial=True)`), the reference's way of listing legal moves.  No board is modified. */
int q2048_legal_moves(const uint8_t *boards, int64_t B, int n, uint8_t *mask_out, void *stream);

/* The canonical image of B 4x4 boards under the eight symmetries (Q2048_FLAG_SYMMETRIC above: images, tie rule, action
 * table): boards_out[i] = the image of boards[i] whose packed key is smallest (bytes are moved, so a tile above 2^15
 * keeps its value; the comparison sees its low nibble, as the state key does), sym_out[i] = g, which image that is.
 * boards_out may be `boards` itself (in place) or NULL, sym_out may be NULL.  What a host that canonicalises for
 * itself needs, and the symbol by which a caller detects that the library folds symmetries.
 * Errors: n = 5 -> Q2048_ERR_UNSUPPORTED (other n too); boards NULL -> Q2048_ERR_NULL; boards or boards_out not 16-byte
 * aligned -> Q2048_ERR_ALIGN; B < 0 -> Q2048_ERR_SIZE.  B == 0: nothing happens, Q2048_OK. */
int q2048_canonicalize(const uint8_t *boards, int64_t B, int n, uint8_t *boards_out, uint8_t *sym_out, void *stream);

/* One-hot state encoder of the reference's DQN front-end (Deep_QLearning/main_dir/
 * Dqn8TestNOPERCNN.py:271-277: one_hot(log2(tile), depth 16) transposed to [16, 4, 4]):
 * out[i][c][r][col] = 1 if the log2 tile at (r, col) equals c (empty cells are channel 0, tiles
 * of 2^16 and above encode as all zeros, as tf.one_hot does), else 0.  4x4 boards;
 * out is float32 (dtype = 0) or bfloat16 (dtype = 1), 16-byte aligned, [B][16][4][4]. */
int q2048_encode_onehot(const uint8_t *boards, int64_t B, int dtype, void *out, void *stream);

/* ---- row-tuple linear Q: BASELINE configs[1], "flat-array Q over row-tuple features" ----------
 * NOT the reference's learner (its Q is keyed by the whole board, Agent/main.py:82) but the same
 * loop with a different table: weights = float[4][65536][4] (16-byte aligned, zero = untrained),
 * Q(s,a) = sum over rows r of weights[r][idx_r(s)][a], idx_r = the row's four log2 nibbles.
 * Same epsilon-greedy / TD target as Agent/main.py:34-43; the error is spread evenly over the
 * four weights, each written as (value read + delta) -- concurrent lanes race per weight and the
 * last writer wins (summing all lanes' deltas would scale the step size by the batch size).
 * 4x4 boards only.
 * A cell >= 16 is not an error on this family: the row index takes each cell's low nibble, so 16 reads the entries
 * of an empty cell and nothing reports it.
 * The family: _choose / _lookup / _update (the four-call loop), _fused_rollout (the learner, `steps` steps per launch)
 * and _play_rollout (the greedy player over the legal moves, `steps` steps per launch, weights only read). */
int q2048_rt_choose(const float *weights, const uint8_t *boards, int64_t B, double eps,
                    uint64_t seed, uint64_t env_id0, uint32_t ctr, uint8_t *actions, void *stream);
int q2048_rt_lookup(const float *weights, const uint8_t *boards, int64_t B, float *q_out,
                    void *stream);
int q2048_rt_update(float *weights, const uint8_t *boards_s, const uint8_t *actions,
                    const float *reward, const uint8_t *boards_s2, const uint8_t *done, int64_t B,
                    double lr, double gamma, uint32_t *status, void *stream);
int q2048_rt_fused_rollout(uint8_t *boards, q2048_aux *aux, float *weights, int64_t B,
                           int64_t steps, double eps, double lr, double gamma, uint64_t seed,
                           uint64_t env_id0, uint32_t ctr0, int64_t *stats_i, double *stats_f,
                           uint32_t *status, void *stream);

/* The GREEDY PLAYER ON WEIGHTS: q2048_play_rollout's loop with a different row source, 4x4 only -- what trained
 * weights are worth when only moves that change the board are made, `steps` steps for B envs in ONE launch.  It
 * replaces the loop rt_lookup / legal_moves / env_step / env_reset(done).  One step of one env (lane i = global env
 * env_id0 + i, counter ctr0 + t):
 *   row     BY DEFINITION what q2048_rt_lookup returns for the board: per action a,
 *           (W[0][i0][a] + W[1][i1][a]) + (W[2][i2][a] + W[3][i3][a]) in float32 with that association, i_r the low
 *           nibbles of row r's four cells (a cell >= 16 aliases, see above);
 *   mask, action, explore, step
 *           exactly q2048_play_rollout's: the trial-move mask of q2048_legal_moves; the first maximum of the row over
 *           the legal moves (ascending, strict >), action 0 with no legal move; the DRAW CONTRACT of the player -- one
 *           Philox call per step, the env explores iff x0 < ceil(eps * 2^32) AND it has a legal move, its move is then
 *           the k-th legal one in ascending order, k = (x1 * n_legal) >> 32, and a step without a legal move is not
 *           counted as explored; x2, x3 of the same call spawn (Q2048_FLAG_ENV_DQN: the DQN path's env, words 0, 1 of
 *           stream 2); on done the episode statistics, then the reset of q2048_fused_rollout.
 * Written: boards, aux and the statistics (steps, valid, explore, episodes, the score / return sums, the max-tile
 * histogram, the reward sum, ADDED to stats_i / stats_f; either may be NULL) -- nothing else.  `weights` is const: all
 * 4 MiB are bit-identical afterwards, and `status` is required and never written.  The result is a function of
 * (weights, boards, aux, seed, env ids, counter) at any B.  On the device the weights are read with plain loads:
 * launches on one stream order them against q2048_rt_fused_rollout / q2048_rt_update.
 * flags: Q2048_FLAG_ENV_DQN, Q2048_FLAG_RESET_SHAPING; any other bit -- Q2048_FLAG_INDEPENDENT and
 * Q2048_FLAG_SYMMETRIC included, neither means anything to weights -- is Q2048_ERR_FLAGS.  Argument errors, checked on
 * the host before anything is launched, in this order: B (Q2048_ERR_SIZE), flags, boards / aux / weights / status NULL,
 * their 16-byte alignment (boards, aux, weights), steps < 0 or > 2^30 (Q2048_ERR_SIZE), eps outside [0, 1]
 * (Q2048_ERR_RANGE).  A refused call writes nothing.  B == 0 or steps == 0: checked, then nothing happens, Q2048_OK. */
int q2048_rt_play_rollout(uint8_t *boards, q2048_aux *aux, const float *weights, int64_t B, int64_t steps,
                          double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                          int64_t *stats_i, double *stats_f, uint32_t *status, void *stream);

/* ---- line-tuple linear Q: the rows AND the columns of the board as features ("all lines") ----------------------
 * The row-tuple family above with eight features instead of four, 4x4 boards only.  weights = float[8][65536][4]
 * (8 MiB, 16-byte aligned, zero = untrained).
 *   features  f = 0..3 is row r = f:       idx_f = sum over k of (cell[4 r + k] & 15) << 4 k -- the row-tuple index;
 *             f = 4..7 is column c = f-4:  idx_f = sum over k of (cell[4 k + c] & 15) << 4 k (cell k of the column,
 *             counted from the top, in nibble k).  A cell >= 16 aliases by the mask, as above, and is not an error.
 *   Q value   Q(s,a) = ((e0 + e1) + (e2 + e3)) + ((e4 + e5) + (e6 + e7)), e_f = weights[f][idx_f][a], in float32 with
 *             exactly that association (the first half is the row-tuple sum of the rows).
 *   TD step   target = (double)reward + gamma * (double)max_a' Q(s',a') * (done ? 0.0 : 1.0);
 *             d = (float)((lr * 0.125) * (target - (double)Q(s,a))), rounded once; each of the eight
 *             weights[f][idx_f(s)][a] is written as (the value this lane gathered) + d: a plain store, the last
 *             writer wins (summing every lane's delta would scale the step size by the batch size, as above).
 *   draws     the epsilon-greedy choice, the draws, the env step and the reset are exactly those of q2048_rt_choose /
 *             q2048_rt_fused_rollout; the player's mask, its argmax over the legal moves and its draw contract are
 *             exactly those of q2048_rt_play_rollout, Q2048_FLAG_ENV_DQN and Q2048_FLAG_RESET_SHAPING included.
 * Each entry point has the argument list of its q2048_rt_* counterpart, checks its arguments in the same order and
 * returns the same codes; `weights` is the 8 MiB array.  Row-tuple weights become line-tuple weights of the same Q
 * by copying them into features 0..3 and zeroing features 4..7. */
int q2048_lt_choose(const float *weights, const uint8_t *boards, int64_t B, double eps,
                    uint64_t seed, uint64_t env_id0, uint32_t ctr, uint8_t *actions, void *stream);
int q2048_lt_lookup(const float *weights, const uint8_t *boards, int64_t B, float *q_out,
                    void *stream);
int q2048_lt_update(float *weights, const uint8_t *boards_s, const uint8_t *actions,
                    const float *reward, const uint8_t *boards_s2, const uint8_t *done, int64_t B,
                    double lr, double gamma, uint32_t *status, void *stream);
int q2048_lt_fused_rollout(uint8_t *boards, q2048_aux *aux, float *weights, int64_t B,
                           int64_t steps, double eps, double lr, double gamma, uint64_t seed,
                           uint64_t env_id0, uint32_t ctr0, int64_t *stats_i, double *stats_f,
                           uint32_t *status, void *stream);
int q2048_lt_play_rollout(uint8_t *boards, q2048_aux *aux, const float *weights, int64_t B, int64_t steps,
                          double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                          int64_t *stats_i, double *stats_f, uint32_t *status, void *stream);

/* ---- afterstate value learner on the line features ---------------------------------------------------------------
 * A third weights family, 4x4 boards only: one VALUE per line entry instead of a Q value per (entry, action), and a
 * state is judged by the four boards its moves lead to before the spawn (the afterstates).
 *   weights   V = float[8][65536] (2 MiB, 16-byte aligned, zero = untrained); feature f is indexed exactly as in the
 *             line-tuple family above (rows 0..3, columns 0..3 from the top, low nibbles; a cell >= 16 aliases).
 *   value     v(x) = ((V[0][i0] + V[1][i1]) + (V[2][i2] + V[3][i3])) + ((V[4][i4] + V[5][i5]) + (V[6][i6] + V[7][i7])),
 *             float32 with exactly that association.
 *   evaluation of a state s, for a = 0..3 (0 left, 1 up, 2 right, 3 down): c_a = s moved by a WITHOUT the spawn,
 *             score_a its merge score, legal_a = the move changes the board; q_a = (float)score_a + v(c_a), one
 *             float32 addition.  A move that does not change the board gives 0 + v(s); there is no special case.
 *   has_move(s) = any legal_a.  best(s) = q_a at the first maximum over the legal moves (strict >, ascending a);
 *             0.0f if there is no legal move.
 *   choice    in EVERY entry point of the family the player's draw contract: greedy = that first maximum over the
 *             legal moves; exploring (x0 below epsilon's threshold, and a legal move exists) = the k-th legal move,
 *             k = (x1 * n_legal) >> 32; no legal move = action 0, not counted as explored.  (Not the unmasked
 *             epsilon-greedy of q2048_lt_choose: an afterstate learner can only learn from moves that change the board.)
 *   TD step   for a transition (s, a, s2, done): x = c_a(s).  If a is not legal in s nothing is written (no error:
 *             it is the step on which the env reports the end of the game).  Otherwise
 *             live = (!done && has_move(s2)) ? 1.0 : 0.0;  target = (gamma * (double)best(s2)) * live;
 *             d = (float)((lr * 0.125) * (target - (double)v(x))), rounded once; each V[f][idx_f(x)] is written as
 *             (the value this lane gathered) + d: a plain 4-byte store, the last writer wins.  The reward of (s, a)
 *             does not enter: v(x) estimates what comes AFTER the move, and the learner's reward is the merge score
 *             of the next move, inside best(s2).  The env's shaped reward still goes into aux and the statistics.
 *   fused     q2048_av_fused_rollout, per lane and step: evaluate s (carried from the previous step), choose with
 *             x0, x1, env step with x2, x3 (default profile, no flags), evaluate s', TD step on c_act with best(s'),
 *             on done statistics + reset + evaluate the new board; otherwise the evaluation of s' is carried, and
 *             every entry of it at a (feature, index) the TD step wrote takes the written value -- so B = 1 is
 *             exactly the four-call loop.  Q2048_ST_EXPLORE counts the steps the choice reports as explored.
 *   player    q2048_av_play_rollout: q2048_lt_play_rollout with the row q_a; weights are only read;
 *             Q2048_FLAG_ENV_DQN and Q2048_FLAG_RESET_SHAPING as there.
 * Argument lists: q2048_av_lookup / _choose / _fused_rollout / _play_rollout have those of their q2048_lt_*
 * counterparts, q2048_av_value that of the lookup with v_out[B], q2048_av_update that of q2048_lt_update without
 * `reward`.  Checks, their order and the codes are the counterparts'; a refused call writes nothing; B == 0 or
 * steps == 0 is Q2048_OK.  q2048_av_update: an action > 3 sets Q2048_STATUS_BAD_ACTION and skips the lane. */
int q2048_av_value(const float *weights, const uint8_t *boards, int64_t B, float *v_out, void *stream);
int q2048_av_lookup(const float *weights, const uint8_t *boards, int64_t B, float *q_out,
                    void *stream);
int q2048_av_choose(const float *weights, const uint8_t *boards, int64_t B, double eps,
                    uint64_t seed, uint64_t env_id0, uint32_t ctr, uint8_t *actions, void *stream);
int q2048_av_update(float *weights, const uint8_t *boards_s, const uint8_t *actions,
                    const uint8_t *boards_s2, const uint8_t *done, int64_t B,
                    double lr, double gamma, uint32_t *status, void *stream);
int q2048_av_fused_rollout(uint8_t *boards, q2048_aux *aux, float *weights, int64_t B,
                           int64_t steps, double eps, double lr, double gamma, uint64_t seed,
                           uint64_t env_id0, uint32_t ctr0, int64_t *stats_i, double *stats_f,
                           uint32_t *status, void *stream);
int q2048_av_play_rollout(uint8_t *boards, q2048_aux *aux, const float *weights, int64_t B, int64_t steps,
                          double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                          int64_t *stats_i, double *stats_f, uint32_t *status, void *stream);

/* ---- 6-tuple afterstate network with shared symmetric weights ---------------------------------------------------
 * A fourth weights family, 4x4 boards only: the afterstate family above with another feature set -- four 6-cell
 * patterns, each read on the eight images of the board, one weight table per pattern shared by the eight images.
 *   weights   V = float[4][16777216] (256 MiB, 16-byte aligned, zero = untrained).  Pattern p has the cells P_p, with
 *             cell index 4r + c:  P0 = {0,1,2,3,4,5}  P1 = {4,5,6,7,8,9}  P2 = {0,1,2,4,5,6}  P3 = {4,5,6,8,9,10}.
 *   images    the eight images of Q2048_FLAG_SYMMETRIC, with the same numbering: img_g(b) = np.rot90(b, g) for
 *             g = 0..3, img_g(b) = np.rot90(np.fliplr(b), g - 4) for g = 4..7.
 *   index     idx[p][g](b) = sum over k = 0..5 of (img_g(b).flat[P_p[k]] & 15) << 4k.  A cell >= 16 aliases by the
 *             mask, as in the other weight families, and is not an error.  Every index is below 2^24 by
 *             construction, so no board can address outside the array.
 *   value     e[p][g] = V[p][idx[p][g](x)];  s_p = ((e[p][0] + e[p][1]) + (e[p][2] + e[p][3])) + ((e[p][4] + e[p][5])
 *             + (e[p][6] + e[p][7]));  v(x) = (s_0 + s_1) + (s_2 + s_3); float32 with exactly that association.
 *   evaluation, has_move, best, choice: word for word those of the afterstate family: q_a = (float)score_a + v(c_a),
 *             no special case for a move that does not change the board, and every entry point uses the player's
 *             draw contract.
 *   TD step   for (s, a, s2, done), x = c_a(s): nothing is written if a is not legal in s; an action > 3 sets
 *             Q2048_STATUS_BAD_ACTION and skips the lane.  live and target are those of the afterstate family;
 *             d = (float)((lr * 0.03125) * (target - (double)v(x))), rounded once.  The lane gathers all 32 entries
 *             of x, then writes each V[p][idx[p][g](x)] as (the value gathered at that entry) + d: plain 4-byte
 *             stores, the last writer wins.  Where several of a lane's 32 entries are the same weight (a board with
 *             a symmetry: the empty board has 4 distinct entries among its 32) they gathered the same value and
 *             store the same value, so that weight moves by d ONCE, not once per occurrence.  This is this family's
 *             rule; it is not the literature's, which adds the error once per occurrence.
 *   fused     q2048_nt_fused_rollout, per lane and step: evaluate s, choose with x0, x1, env step with x2, x3
 *             (default profile, no flags), evaluate s', TD step on c_act, on done statistics + reset.  Nothing is
 *             carried from step to step: s is evaluated from memory on every step and the 32 entries of c_act are
 *             gathered again for the TD step, so every evaluation a lane makes sees the lane's own earlier writes
 *             and B = 1 is exactly the four-call loop, all 256 MiB bit for bit.
 *   player    q2048_nt_play_rollout: q2048_av_play_rollout with this row; weights are only read;
 *             Q2048_FLAG_ENV_DQN and Q2048_FLAG_RESET_SHAPING as there.
 * Each entry point has the argument list of its q2048_av_* counterpart, the same checks in the same order and the
 * same codes; a refused call writes nothing; B == 0 or steps == 0 is Q2048_OK. */
int q2048_nt_value(const float *weights, const uint8_t *boards, int64_t B, float *v_out, void *stream);
int q2048_nt_lookup(const float *weights, const uint8_t *boards, int64_t B, float *q_out,
                    void *stream);
int q2048_nt_choose(const float *weights, const uint8_t *boards, int64_t B, double eps,
                    uint64_t seed, uint64_t env_id0, uint32_t ctr, uint8_t *actions, void *stream);
int q2048_nt_update(float *weights, const uint8_t *boards_s, const uint8_t *actions,
                    const uint8_t *boards_s2, const uint8_t *done, int64_t B,
                    double lr, double gamma, uint32_t *status, void *stream);
int q2048_nt_fused_rollout(uint8_t *boards, q2048_aux *aux, float *weights, int64_t B,
                           int64_t steps, double eps, double lr, double gamma, uint64_t seed,
                           uint64_t env_id0, uint32_t ctr0, int64_t *stats_i, double *stats_f,
                           uint32_t *status, void *stream);
int q2048_nt_play_rollout(uint8_t *boards, q2048_aux *aux, const float *weights, int64_t B, int64_t steps,
                          double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                          int64_t *stats_i, double *stats_f, uint32_t *status, void *stream);

/* ---- temporal-coherence step sizes for the 6-tuple afterstate network --------------------------------------------
 * The network's learner with a step size of its own per weight (TC learning): a weight learns at full rate while its
 * TD errors agree in sign and stops by itself as they cancel.
 *   weights   V = float[4][16777216] of the family above, unchanged: every q2048_nt_* reader works on a V trained here.
 *   acc       float[4][16777216][2] (512 MiB, 16-byte aligned) beside it: acc[p][idx] = {E, A}, the signed sum of the
 *             TD errors the weight V[p][idx] has seen and the sum of their magnitudes.  All zero = no history.  A pair
 *             is 8 bytes, 8-byte aligned, always read with one 8-byte load and written with one 8-byte store: a
 *             reader never sees the E of one writer with the A of another.
 *   TD step   for (s, a, s2, done), x = c_a(s), with q2048_nt_update's skip rules (an action > 3 sets
 *             Q2048_STATUS_BAD_ACTION and skips the lane; an action that does not change s writes nothing).  The lane
 *             gathers the 32 entries of x from V and the 32 pairs of x from acc.  live and target are those of the
 *             afterstate family;  err = target - (double)v(x), in double;  e = (float)err, rounded once.  Per entry i:
 *               r_i = (A_i > 0.0f) ? fminf(fabsf(E_i) / A_i, 1.0f) : 1.0f      one IEEE float32 division; in [0, 1] for
 *                     ANY contents of acc (a loaded file's included), and 1 where a NaN is involved;
 *               d_i = (float)(((lr * 0.03125) * err) * (double)r_i)             rounded once, no contraction.
 *             Then V[p][idx] = (the value gathered there) + d_i and acc[p][idx] = {E_i + e, A_i + fabsf(e)}: plain
 *             stores, the last writer wins.  Entries of one lane that are the same weight gathered the same values and
 *             store the same values, so that weight and its pair move ONCE (the family's rule).
 *   (a)       On an all-zero acc every r_i is 1 and d_i is bit for bit q2048_nt_update's d: one step from no history
 *             is the plain step.
 *   (b)       |E| <= A holds exactly for every pair ever stored, racing lanes included: it holds for zero;
 *             |E + e| <= A + |e| holds in exact arithmetic; rounding to nearest is monotone and symmetric; and every
 *             stored pair derives from ONE untorn pair.
 *   fused     q2048_nt_tc_fused_rollout is q2048_nt_fused_rollout step for step -- evaluation from memory, the
 *             player's draw contract, env step, statistics, reset -- with this TD step; nothing is carried between
 *             steps, so B = 1 is exactly the four-call loop q2048_nt_choose / env step / q2048_nt_tc_update / reset
 *             on all 768 MiB, and lr = 0 leaves V bit-identical while acc accumulates.
 * Argument checks are the q2048_nt_* counterpart's in its order, with acc checked for NULL and for 16-byte alignment
 * directly after weights; then, after the alignment checks, Q2048_ERR_RANGE if the byte ranges of weights (256 MiB)
 * and acc (512 MiB) overlap.  A refused call writes nothing; B == 0 or steps == 0 is Q2048_OK. */
int q2048_nt_tc_update(float *weights, float *acc, const uint8_t *boards_s, const uint8_t *actions,
                       const uint8_t *boards_s2, const uint8_t *done, int64_t B,
                       double lr, double gamma, uint32_t *status, void *stream);
int q2048_nt_tc_fused_rollout(uint8_t *boards, q2048_aux *aux, float *weights, float *acc, int64_t B,
                              int64_t steps, double eps, double lr, double gamma, uint64_t seed,
                              uint64_t env_id0, uint32_t ctr0, int64_t *stats_i, double *stats_f,
                              uint32_t *status, void *stream);

/* ---- TD(lambda) for the 6-tuple network: a truncated eligibility trace per lane (q2048_nt_lambda_*) ---------------
 * The TD error of a step also moves the last n <= h <= 3 afterstates the lane learned on in the current episode.
 *   weights   V = float[4][16777216] of the family above, unchanged: every q2048_nt_* reader works on a V trained here.
 *   trace     uint64_t[B][4], 32 bytes per lane, 16-byte aligned, caller-owned; lane i uses trace[i].  Word 0 is n,
 *             words 1..3 are the packed keys (cell 4r + c in nibble 4r + c) of x_{t-1}, x_{t-2}, x_{t-3}, newest
 *             first.  Every word beyond n is 0 in what these entry points store, so the array compares byte for byte;
 *             all zero = no history.  (On input n is read as min(n, 3) and the keys as they are: more than h keys are
 *             updated once and truncated by the push.)  h == 0: never read or written, may be NULL.
 *   TD step   on an afterstate x with the evaluation of the next state, `done` and a flag `cut`, in this order:
 *             1. cut: n = 0 and the three keys 0 (Watkins' cut: the error of an explored move says nothing about the
 *                afterstates before it);
 *             2. err = target - (double)v(x), live, target and gather those of q2048_nt_update;
 *             3. d_0 = (float)((lr * 0.03125) * err), q2048_nt_update's d bit for bit; the 32 entries of x are written
 *                as gathered + d_0 (a weight x reads several times moves once: the family's rule);
 *             4. for k = 1..n in ascending order, each after the stores of k - 1: the 32 entries of key k are gathered
 *                and each is stored as gathered + d_k, d_k = (float)(((lr * 0.03125) * L_k) * err), L_1 = lambda,
 *                L_2 = lambda * lambda, L_3 = (lambda * lambda) * lambda in double, no contraction; nothing is summed.
 *                A weight x shares with an earlier afterstate moves by d_0 and then by d_k;
 *             5. push: the keys become (key(x), key_1, key_2) truncated to h words, n = min(n + 1, h);
 *             6. done: the lane's four words are zeroed.
 *             h == 0 is step 3 alone: q2048_nt_update / q2048_nt_fused_rollout byte for byte.
 *   update    q2048_nt_lambda_update has q2048_nt_update's skip rules: an action > 3 sets Q2048_STATUS_BAD_ACTION and
 *             skips the lane; an action that does not change s writes no weight and pushes nothing -- but a set `done`
 *             still zeroes the lane's trace (the env reports the end of a game on exactly such a step, and a trace
 *             never crosses an episode).  cut[i] != 0 is the flag of lane i; cut == NULL: no cuts.
 *   fused     q2048_nt_lambda_fused_rollout is q2048_nt_fused_rollout step for step -- evaluation from memory on every
 *             step, draws, env step, statistics, reset -- with this TD step and cut = the `explored` flag of the
 *             step's choice.  The trace is loaded at launch and stored at the end, so launches chain, and B = 1 is
 *             exactly the loop q2048_nt_choose_ex / env step / q2048_nt_lambda_update / reset.
 *   choose_ex q2048_nt_choose with the `explored` flag of the draw contract per lane (0 / 1; may be NULL).
 * Argument checks are the q2048_nt_* counterpart's in its order, with trace checked for NULL (unless h == 0) and for
 * 16-byte alignment directly after weights; last, Q2048_ERR_RANGE for h outside 0..3 or lambda outside [0, 1] or not
 * finite.  A refused call writes nothing; B == 0 or steps == 0 is Q2048_OK. */
int q2048_nt_choose_ex(const float *weights, const uint8_t *boards, int64_t B, double eps,
                       uint64_t seed, uint64_t env_id0, uint32_t ctr, uint8_t *actions,
                       uint8_t *explored, void *stream);
int q2048_nt_lambda_update(float *weights, uint64_t *trace, const uint8_t *boards_s, const uint8_t *actions,
                           const uint8_t *boards_s2, const uint8_t *done, const uint8_t *cut, int64_t B,
                           double lr, double gamma, double lambda, int h, uint32_t *status, void *stream);
int q2048_nt_lambda_fused_rollout(uint8_t *boards, q2048_aux *aux, float *weights, uint64_t *trace, int64_t B,
                                  int64_t steps, double eps, double lr, double gamma, double lambda, int h,
                                  uint64_t seed, uint64_t env_id0, uint32_t ctr0, int64_t *stats_i,
                                  double *stats_f, uint32_t *status, void *stream);

/* ---- the synchronous batch step of the 6-tuple network: reproducible training (q2048_nt_sync_*) --------------------
 * In one step every lane evaluates against the same frozen weights, the TD errors that fall on a weight are summed
 * exactly, as integers, and the weight then moves once, by the mean of those errors.  The result is a pure function
 * of the inputs: it does not depend on scheduling, on the number of threads or on which lane arrives first, and it
 * is the same bytes on the device and in the CPU twin.
 *   weights   V = float[4][16777216] of the family above, unchanged: every q2048_nt_* reader works on a V trained here.
 *   acc       uint64_t[4][16777216][2], 1 GiB, 16-byte aligned, caller-owned; acc[p][idx] = {S, C}: the two's-complement
 *             sum of the quantised errors of weight idx of pattern p and the number of contributions.  It must be all
 *             zero on entry (not checked) and is all zero again when a call returns: it is never saved.
 *   pend      (fused only) uint64_t[B], 16-byte aligned, caller-owned scratch: the packed key (cell 4r + c in nibble
 *             4r + c) of the afterstate each lane learned on in the current step.  Ignored on entry, every word 0 on
 *             return.  An afterstate of a legal move is never the empty board, so key 0 is "none".
 *   phase A   V is only read.  A lane with a TD sample (x, s', done) forms live, target and
 *             err = target - (double)v(x) in double, exactly as q2048_nt_update does, and quantises it:
 *             q = isnan(err) ? 0 : llrint(clamp(err, -262144.0, 262144.0) * 4096.0) -- the product is exact, the
 *             rounding to nearest even.  For each of its 32 entries, PER OCCURRENCE, S += q and C += 1: a weight a
 *             symmetric board reads m times receives m * q and m, so a lone lane still moves it once (the family's
 *             rule).  With B <= 2^20, |S| <= 2^53 and C <= 2^23: exact in double, and nothing wraps.
 *   phase B   after every lane of phase A.  Every weight with C != 0 is written exactly once:
 *             m = (double)S / ((double)C * 4096.0), one IEEE division; d = (float)((lr * 0.03125) * m), rounded once,
 *             no contraction; V[p][idx] = V[p][idx] + d; the pair is zeroed.  Weights with C == 0 are not touched.
 *   update    q2048_nt_sync_update has q2048_nt_update's skip rules (an action > 3 sets Q2048_STATUS_BAD_ACTION and
 *             the lane contributes nothing; a move that does not change s contributes nothing); it is one phase A
 *             over the batch, then one phase B.
 *   fused     q2048_nt_sync_fused_rollout is q2048_nt_fused_rollout step for step with the same draws ctr0 + t --
 *             evaluation of s from memory, the draw contract, env step, evaluation of s', statistics, reset -- with
 *             the TD write replaced by a phase-A contribution and a phase B after every step.  So at ANY B it is
 *             exactly the loop q2048_nt_choose / env step / q2048_nt_sync_update / reset, and steps = n in one call
 *             equals any split of n over several calls.  On the device a step is two launches on `stream`.
 * Argument checks are the q2048_nt_* counterpart's in its order, with acc (then pend) checked for NULL and for 16-byte
 * alignment directly after weights; after the alignment checks, Q2048_ERR_RANGE for B > 1048576 and for overlapping
 * byte ranges of weights and acc.  A refused call writes nothing; B == 0 or steps == 0 is Q2048_OK and writes nothing. */
int q2048_nt_sync_update(float *weights, uint64_t *acc, const uint8_t *boards_s, const uint8_t *actions,
                         const uint8_t *boards_s2, const uint8_t *done, int64_t B, double lr, double gamma,
                         uint32_t *status, void *stream);
int q2048_nt_sync_fused_rollout(uint8_t *boards, q2048_aux *aux, float *weights, uint64_t *acc, uint64_t *pend,
                                int64_t B, int64_t steps, double eps, double lr, double gamma, uint64_t seed,
                                uint64_t env_id0, uint32_t ctr0, int64_t *stats_i, double *stats_f,
                                uint32_t *status, void *stream);

/* ---- one-level expectimax over the spawn, for both afterstate families -------------------------------------------
 * The SEARCHED ROW of a state s replaces q_a = score_a + v(c_a) by the mean of best over the spawns of c_a.  For
 * a = 0..3, with c_a, score_a, legal_a and best as the family defines them above:
 *   a not legal   Q_a = 0.0f; nothing is evaluated for it.
 *   a legal       c_a has n >= 1 empty cells (n <= 15).  For each empty cell j of c_a in ascending row-major order:
 *                 b2_j = best(c_a with a 2 at j), b4_j = best(c_a with a 4 at j), t_j = 9.0 * (double)b2_j + (double)b4_j;
 *                 S_a = ((0.0 + t_j0) + t_j1) + ...: double additions in exactly that order;
 *                 E_a = (float)(S_a / (double)(10 * n)): one IEEE double division, rounded to float32 once;
 *                 Q_a = (float)score_a + E_a: one float32 addition.
 * The weights 9 : 1 stand for the env's spawn rule (a 4 when the draw is >= 3865470567, i.e. with probability
 * 0.1 - 0.6 * 2^-32); the 2^-32-sized difference is ignored.  A state has at most 4 * 15 * 2 = 120 chance nodes.
 *   q2048_{av,nt}_search_lookup        writes the searched row to q_out[B][4] and the mask of the legal moves (bit a)
 *                 to legal_out[B], which is required.  Arguments are checked as by q2048_{av,nt}_lookup.
 *   q2048_{av,nt}_search_play_rollout  q2048_{av,nt}_play_rollout -- argument list, checks, codes, flags, draws
 *                 (x0, x1 choice; x2, x3 spawn; the DQN profile's second spawn from stream 2), statistics, episode
 *                 handling -- with the searched row handed to the choice: the first maximum over the legal moves, or
 *                 the k-th legal move when exploring; no legal move = action 0, not explored.
 * The weights are only read.  The device evaluates the chance nodes of a board on the lanes of one wave and sums them
 * in the order above, so both libraries give the same bits.  A refused call writes nothing; B == 0 or steps == 0 is
 * Q2048_OK. */
int q2048_av_search_lookup(const float *weights, const uint8_t *boards, int64_t B, float *q_out,
                           uint8_t *legal_out, void *stream);
int q2048_av_search_play_rollout(uint8_t *boards, q2048_aux *aux, const float *weights, int64_t B, int64_t steps,
                                 double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                                 int64_t *stats_i, double *stats_f, uint32_t *status, void *stream);
int q2048_nt_search_lookup(const float *weights, const uint8_t *boards, int64_t B, float *q_out,
                           uint8_t *legal_out, void *stream);
int q2048_nt_search_play_rollout(uint8_t *boards, q2048_aux *aux, const float *weights, int64_t B, int64_t steps,
                                 double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                                 int64_t *stats_i, double *stats_f, uint32_t *status, void *stream);

/* ---- two-level expectimax: the searched row with a depth ---------------------------------------------------------
 * Take c_a, score_a, legal_a and the family's best (call it best_0) as defined above.  For d >= 1 the DEPTH-d ROW of a
 * state s is the searched row above with best_{d-1} in place of best:
 *   a not legal   Q^d_a = 0.0f; nothing is evaluated for it.
 *   a legal       for each empty cell j of c_a in ascending row-major order:
 *                 t_j = 9.0 * (double)best_{d-1}(c_a with a 2 at j) + (double)best_{d-1}(c_a with a 4 at j);
 *                 S_a = ((0.0 + t_j0) + t_j1) + ...: double additions in exactly that order;
 *                 E_a = (float)(S_a / (double)(10 * n)); Q^d_a = (float)score_a + E_a.
 *   best_d(x)     the depth-d row of x at the first maximum over the legal moves of x; 0.0f for a state without a legal
 *                 move, and nothing is evaluated beneath such a state.
 * Depth 1 is the searched row above, bit for bit.  Depth 2 evaluates at most 120 level-one nodes with at most 120
 * leaves each: 14,400 evaluations of the family per state.  The order of every S sum, at both levels, is part of the
 * contract: the device gives a board a block, spreads its level-one nodes over the block's waves and the leaves of a
 * node over the lanes of a wave, and sums both levels in the order above, so both libraries give the same bits.
 *   q2048_{av,nt}_search_lookup_depth        q2048_{av,nt}_search_lookup with `depth` after B.
 *   q2048_{av,nt}_search_play_rollout_depth  q2048_{av,nt}_search_play_rollout with `depth` after steps: draws, flags,
 *                 env profiles, statistics and episode handling unchanged.
 * depth outside {1, 2} is Q2048_ERR_RANGE, checked before every other argument; then the checks of the function without
 * a depth, in its order, with its codes.  With depth == 1 they ARE those functions (the same kernels, the same bytes).
 * The weights are only read.  A refused call writes nothing; B == 0 or steps == 0 is Q2048_OK. */
int q2048_av_search_lookup_depth(const float *weights, const uint8_t *boards, int64_t B, int depth, float *q_out,
                                 uint8_t *legal_out, void *stream);
int q2048_av_search_play_rollout_depth(uint8_t *boards, q2048_aux *aux, const float *weights, int64_t B, int64_t steps,
                                       int depth, double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0,
                                       uint32_t flags, int64_t *stats_i, double *stats_f, uint32_t *status,
                                       void *stream);
int q2048_nt_search_lookup_depth(const float *weights, const uint8_t *boards, int64_t B, int depth, float *q_out,
                                 uint8_t *legal_out, void *stream);
int q2048_nt_search_play_rollout_depth(uint8_t *boards, q2048_aux *aux, const float *weights, int64_t B, int64_t steps,
                                       int depth, double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0,
                                       uint32_t flags, int64_t *stats_i, double *stats_f, uint32_t *status,
                                       void *stream);

/* ---- the staged network: a weight table per largest-tile stage (q2048_nts_*) --------------------------------------
 * The 6-tuple network above with one set of weights per stage of the game: weights = float32 [S][4][16777216],
 * 1 <= S <= 8 (256 MiB per stage).  Arrived without an ABI bump, detected by its symbols.
 *   stages    the thresholds as nibbles: nibble i is t_{i+1}, a tile exponent in 1..15 (the tile 2^t).  The thresholds
 *             ascend strictly, the nonzero nibbles are contiguous from nibble 0, the top nibble is 0 (at most seven
 *             thresholds); S = 1 + the number of nonzero nibbles.  stages == 0 is the plain network: every q2048_nts_*
 *             function then gives what its q2048_nt_* counterpart gives, byte for byte.  Any other word is
 *             Q2048_ERR_RANGE, checked before every other argument.
 *   stage(x)  the number of thresholds t_i with maxnib(x) >= t_i, maxnib(x) = the largest nibble of the packed key of
 *             x (a cell >= 16 aliases by its low nibble, as in the indices).
 *   v(x)      the network's v over the 32 entries of x taken from table stage(x).  In the evaluation of a state every
 *             candidate afterstate uses its OWN stage: a merge that creates a threshold tile puts that candidate in the
 *             next table while its siblings stay below.  q_a, best, the choice, live and target are the afterstate
 *             family's.
 *   TD step   q2048_nt_update's on table stage(c_act): the 32 entries are gathered from that table and written back as
 *             gathered + d; the target is the best of the staged evaluation of the next state.  A weight that a
 *             symmetric board reads several times moves once, as in the plain network.
 * The nine functions have the argument lists of their q2048_nt_* counterparts with `stages` directly after `weights`,
 * their checks in their order after the spec, their draws, flags, statistics and episode handling.  depth is 1 or 2.
 *   q2048_nts_promote   BULK PROMOTION from stage `from` to stage `to`, on every (p, idx): if the bit pattern of
 *             V[to][p][idx] is 0x00000000 and that of V[from][p][idx] is not, V[to][p][idx] takes the bits of
 *             V[from][p][idx] (a NaN included).  -0.0f counts as written and is never overwritten.  count_out: device
 *             int64, may be NULL; receives the number of entries copied.  Errors, in this order: a malformed spec ->
 *             Q2048_ERR_RANGE; weights NULL -> Q2048_ERR_NULL; not 16-byte aligned -> Q2048_ERR_ALIGN; from == to, or
 *             either outside 0..S-1 -> Q2048_ERR_RANGE.  Stream-ordered; nothing else may touch the two tables while
 *             it runs.  This is not the literature's promote-on-first-access: a weight copied early does not follow
 *             what its source learns later, and the evaluation carries no sentinel test and no second load.
 * A refused call writes nothing; B == 0 or steps == 0 is Q2048_OK. */
int q2048_nts_value(const float *weights, uint32_t stages, const uint8_t *boards, int64_t B, float *v_out,
                    void *stream);
int q2048_nts_lookup(const float *weights, uint32_t stages, const uint8_t *boards, int64_t B, float *q_out,
                     void *stream);
int q2048_nts_choose(const float *weights, uint32_t stages, const uint8_t *boards, int64_t B, double eps,
                     uint64_t seed, uint64_t env_id0, uint32_t ctr, uint8_t *actions, void *stream);
int q2048_nts_update(float *weights, uint32_t stages, const uint8_t *boards_s, const uint8_t *actions,
                     const uint8_t *boards_s2, const uint8_t *done, int64_t B, double lr, double gamma,
                     uint32_t *status, void *stream);
int q2048_nts_fused_rollout(uint8_t *boards, q2048_aux *aux, float *weights, uint32_t stages, int64_t B,
                            int64_t steps, double eps, double lr, double gamma, uint64_t seed, uint64_t env_id0,
                            uint32_t ctr0, int64_t *stats_i, double *stats_f, uint32_t *status, void *stream);
int q2048_nts_play_rollout(uint8_t *boards, q2048_aux *aux, const float *weights, uint32_t stages, int64_t B,
                           int64_t steps, double eps, uint64_t seed, uint64_t env_id0, uint32_t ctr0, uint32_t flags,
                           int64_t *stats_i, double *stats_f, uint32_t *status, void *stream);
int q2048_nts_search_lookup_depth(const float *weights, uint32_t stages, const uint8_t *boards, int64_t B, int depth,
                                  float *q_out, uint8_t *legal_out, void *stream);
int q2048_nts_search_play_rollout_depth(uint8_t *boards, q2048_aux *aux, const float *weights, uint32_t stages,
                                        int64_t B, int64_t steps, int depth, double eps, uint64_t seed,
                                        uint64_t env_id0, uint32_t ctr0, uint32_t flags, int64_t *stats_i,
                                        double *stats_f, uint32_t *status, void *stream);
int q2048_nts_promote(float *weights, uint32_t stages, int from, int to, int64_t *count_out, void *stream);

/* CAROUSEL SHAPING for the staged network: training episodes start in turn at the beginning of every stage, from a pool
 * of boards on which earlier games entered that stage.  Two functions, additive (the ABI version stays; detect them by
 * their symbols).  `stages` is the spec of q2048_nts_*, S its number of stages.
 *   pool      uint8 [S][P][32], 16-byte aligned: a ring of P >= 1 records per stage.  Row 0 is never read or written.
 *   counts    uint64 [S]: counts[k] = records ever committed to stage k; n_k = min(counts[k], P) records are valid, in
 *             slots 0 .. n_k-1.
 *   fresh     uint8 [S][B][32], 16-byte aligned: one record per (stage, lane), written by the learner, consumed by the
 *             commit.  Start it at zero.
 *   record    32 bytes: the board (0..15), aux.score (int32, 16..19), the bits of aux.ep_return (20..23), zero
 *             (24..31).  A record whose 16 board bytes are zero is EMPTY.
 *   q2048_car_fused_rollout   q2048_nts_fused_rollout with two changes.  RECORDING: if a step does not end the game and
 *             leaves a board (spawn included) of a later stage k1 than the one it started from, fresh[k1][lane] takes
 *             the record of the board and aux as the step left them; a later crossing of the lane into the same stage
 *             in the same call overwrites it, a jump over a stage records at k1 only, a restart records nothing.
 *             RESTART: aux.episode += 1 and the four reset draws are taken as always; k = aux.episode % S; if k == 0 or
 *             n_k == 0 the episode starts from an empty board exactly as in q2048_nts_fused_rollout, otherwise board,
 *             score and ep_return come from pool[k][(x0 * n_k) >> 32], x0 the first reset draw.  The pool and the
 *             counts are only read; a lane writes only its own fresh[.][lane].  stages == 0 gives
 *             q2048_nts_fused_rollout's bytes.
 *   q2048_car_commit   for each stage k = 1 .. S-1: the lanes with a non-empty fresh[k][i], in ascending i, m of them;
 *             the record of rank r goes to pool[k][(counts[k] + r) % P] if r + P >= m (of more than P records the last
 *             P land, each in a slot of its own); counts[k] += m; every consumed fresh[k][i] is zeroed whole.
 *             Stream-ordered after the learner on the same stream.
 * Errors, in this order: a malformed spec -> Q2048_ERR_RANGE; a NULL pointer (status included) -> Q2048_ERR_NULL; boards,
 * aux, weights, pool or fresh not 16-byte aligned, counts not 8-byte aligned -> Q2048_ERR_ALIGN; P < 1 or P > 2^32, B or
 * steps out of range -> Q2048_ERR_SIZE; eps outside [0, 1], lr or gamma NaN -> Q2048_ERR_RANGE.  A refused call writes
 * nothing; B == 0 or steps == 0 is Q2048_OK and writes nothing. */
int q2048_car_fused_rollout(uint8_t *boards, q2048_aux *aux, float *weights, uint32_t stages, const uint8_t *pool,
                            const uint64_t *counts, uint8_t *fresh, int64_t P, int64_t B, int64_t steps, double eps,
                            double lr, double gamma, uint64_t seed, uint64_t env_id0, uint32_t ctr0, int64_t *stats_i,
                            double *stats_f, uint32_t *status, void *stream);
int q2048_car_commit(uint8_t *pool, uint64_t *counts, uint8_t *fresh, uint32_t stages, int64_t P, int64_t B,
                     void *stream);

/* Inverse of q2048_table_export (resume / load a table trained elsewhere): inserts `rows`
 * (key, q[4]) pairs into the table, key_words as above.  A key already present has its row
 * overwritten in place (its slot and key words stay, the four values change); a row that finds no slot
 * within the probe limit (2^14 positions of its sequence, or the whole table) sets Q2048_STATUS_TABLE_FULL
 * and is left out, the others are placed.
 * THE SAME KEY MORE THAN ONCE IN ONE CALL leaves exactly one row.  The rows of a call are inserted
 * concurrently and a row's four values are written one by one, so each of the four values of that row is
 * the corresponding value of ONE of the duplicates -- not necessarily all four of the same one, and not
 * necessarily the last in the input.  A caller that needs a particular duplicate to win removes the others
 * first (or imports them in separate calls on one stream: the later call overwrites). */
int q2048_table_import(q2048_slot *table, int cap_log2, const uint64_t *keys, const float *q,
                       int64_t rows, int key_words, uint32_t *status, void *stream);

/* Combines two tables on the device: every occupied row of `src` finds or creates its row in `dst` and is combined with
 * it -- the replicas of a job (one table per rank, dist.py) or two checkpoints become the one table they trained,
 * without a trip through the host.  No reference counterpart (its q_table is one dict in one process); the reading of
 * a state WITHOUT a row is the defaultdict's (Agent/main.py:16): the zero row.  One streaming pass over `src` (the
 * growth's move: 16-byte head of every slot, second half of the occupied ones, find-or-create at the key's home in
 * `dst`); a row that was already in `dst` costs one more read of its values.  key_words as q2048_table_export.
 *   mode, w   Q2048_MERGE_ADD     q_dst = q_dst + w * q_src; a created row holds w * q_src.  w = 1: the sum; K calls
 *                                 with w = 1/K into an empty table: the mean over K replicas.  Any finite w.
 *             Q2048_MERGE_BLEND   key in both: q_dst = (1 - w) * q_dst + w * q_src; key only in src: q_src as it is.
 *                                 w in [0, 1]; 0 keeps the rows dst has and adds the ones it lacks, 1 takes src's.
 *             Q2048_MERGE_MAXABS  per action the value of larger magnitude (q_src if |q_src| > |q_dst|, else q_dst:
 *                                 an untrained entry is exactly 0); a created row holds q_src; w is not used.
 *             Arithmetic: float32, every product and every sum rounded on its own (no fused multiply-add), 1 - w
 *             computed once on the host in float32 -- a float32 model on the host gives the same bits.  (0 * x and
 *             x + 0 are x's own bits for every finite x but -0.0, which comes out as +0.0.)
 *   counters  device uint64[4], ADDED to: [0] occupied src rows read, [1] rows created in dst, [2] rows combined with
 *             an existing dst row, [3] rows dropped (no slot within the probe limit); [0] = [1] + [2] + [3].
 *   status    may be NULL.  Q2048_STATUS_TABLE_FULL when a row was dropped, Q2048_STATUS_DEEP_ROW when a created row
 *             lies beyond the learning paths' probe limit (as q2048_table_import).
 * Stream-ordered.  Nothing else may write `src` or touch `dst` while the call is in flight; `src` is never written.
 * The call creates rows in `dst`: its line summaries, in the slots or beside the table, are stale afterwards and must be
 * written again before Q2048_FLAG_LINE_SUMMARY is passed again.  The `reserved` words of 4x4 slots (key_words = 1) are
 * neither read nor written: a summary word in `src` is ignored, the word of a created row stays what it was (0 in a
 * table without summaries).  Keys salted by Q2048_FLAG_INDEPENDENT merge key by key like any others, which is rarely
 * meaningful: the same env id has to mean the same learner in both tables.
 * Errors, in this order: dst, src or counters NULL -> Q2048_ERR_NULL; a cap_log2 outside 4..40 or key_words not 1 or 2
 * -> Q2048_ERR_SIZE; a table not 16-byte aligned -> Q2048_ERR_ALIGN; an unknown mode -> Q2048_ERR_FLAGS; w not finite,
 * or outside [0, 1] with Q2048_MERGE_BLEND -> Q2048_ERR_RANGE; the two tables' byte ranges overlap (src == dst
 * included) -> Q2048_ERR_RANGE. */
#define Q2048_MERGE_ADD 0
#define Q2048_MERGE_BLEND 1
#define Q2048_MERGE_MAXABS 2
int q2048_table_merge(q2048_slot *dst, int dst_cap_log2, const q2048_slot *src, int src_cap_log2,
                      int key_words, int mode, float w, uint64_t *counters, uint32_t *status, void *stream);

/* Folds a PLAIN table into a SYMMETRY-FOLDED one on the device (Q2048_FLAG_SYMMETRIC above: images, canonical image,
 * pi_g): the way into a folded table for a learner that was trained plain.  `src` is a plain 4x4 table, `dst` a folded
 * one that may already hold rows.  The rows of a board's up to eight mirror images become ONE row, combined by `fold`,
 * and that row finds or creates the row of the canonical key in `dst`, combined with it by `mode` and `w` exactly as
 * q2048_table_merge combines a source row (its arithmetic, its created-row rule, its status bits).  The merge's
 * sibling; arrived without an ABI bump, detected by its symbol.  The result depends on the two tables' ROWS only --
 * not on slot positions, not on scheduling -- and a float32 model on the host gives the same bits.
 *   ORBIT     For a source key m, c = the canonical key of m.  The MEMBERS of c's orbit are image_h(c), h = 0..7, in
 *             ascending h; an h whose key equals that of a smaller h is skipped (boards with a stabiliser have 4, 2 or
 *             1 distinct images).  The PRESENT members are the ones that have a row in `src`.
 *   FRAME     A member's row enters the canonical frame by the member's own g -- the smallest g with
 *             image_g(member) = c, the convention of the fused rollout when it meets that board:
 *             Qc[pi_g(a)] = Q_member[a].
 *   fold      The present members' canonical-frame rows are combined per action, in member order.  float32, every sum
 *             and every product rounded on its own; the first entry that joins is taken as it is (no 0 + x); the mean's
 *             division is a multiplication by the constant float32(1.0 / k), k = 1..8.
 *             Q2048_FOLD_MEAN          the sum over the k present members, times float32(1.0 / k).
 *             Q2048_FOLD_MEAN_TRAINED  per action the same over the members whose entry is not exactly 0 (+0 or -0),
 *                                      k counting those; +0 when none is -- an untrained entry does not dilute a
 *                                      trained one.
 *             Q2048_FOLD_SUM           the sum over the present members.
 *             Q2048_FOLD_MAXABS        per action the entry of larger magnitude; on equal magnitude the earlier
 *                                      member's.
 *   mode, w   as q2048_table_merge, with the orbit's row in the place of the source row.
 *   counters  device uint64[5], ADDED to: [0] occupied src rows read, [1] orbits (each has exactly one leading row),
 *             [2] rows created in dst, [3] rows combined with an existing dst row, [4] orbits dropped (no slot within
 *             the probe limit); [1] = [2] + [3] + [4].
 *   status    may be NULL; Q2048_STATUS_TABLE_FULL / Q2048_STATUS_DEEP_ROW as q2048_table_merge.
 * One streaming pass over `src`, and for every occupied slot lookups of the orbit's other members in `src` (up to the
 * bulk probe limit of 2^14 positions): a row that finds a present member ahead of itself stops, the orbit's first
 * present member collects the rest and performs the orbit's one write, so exactly one lane writes each dst row and no
 * float atomic is needed.  Stream-ordered.  Nothing else may write `src` or touch `dst` while the call is in flight.
 * `src` is never written and its `reserved` words are never read (line summaries in it are harmless); the `reserved`
 * words of `dst` are untouched, and its line summaries are stale afterwards, as after a merge.  Keys salted by
 * Q2048_FLAG_INDEPENDENT cannot be told from board keys: they fold to nonsense, and the caller must not pass them.
 * Errors, in this order: dst, src or counters NULL -> Q2048_ERR_NULL; key_words == 2 -> Q2048_ERR_UNSUPPORTED (5x5 has
 * no folded table); key_words not 1 or 2, or a cap_log2 outside 4..40 -> Q2048_ERR_SIZE; a table not 16-byte aligned
 * -> Q2048_ERR_ALIGN; an unknown fold or mode -> Q2048_ERR_FLAGS; w not finite, or outside [0, 1] with
 * Q2048_MERGE_BLEND -> Q2048_ERR_RANGE; the two tables' byte ranges overlap -> Q2048_ERR_RANGE. */
#define Q2048_FOLD_MEAN 0
#define Q2048_FOLD_MEAN_TRAINED 1
#define Q2048_FOLD_SUM 2
#define Q2048_FOLD_MAXABS 3
int q2048_table_fold(q2048_slot *dst, int dst_cap_log2, const q2048_slot *src, int src_cap_log2, int key_words,
                     int fold, int mode, float w, uint64_t *counters, uint32_t *status, void *stream);

/* Unfolds a SYMMETRY-FOLDED table into a PLAIN one on the device: the fold's inverse, and the way out of a folded table
 * for every path that only understands plain ones (q2048_q_choose / _update, q2048_det_rollout, the reference's own
 * loop over an exported dict).  `src` is a symmetry-folded 4x4 table, `dst` a plain one that may already hold rows
 * (Q2048_FLAG_SYMMETRIC above: images, canonical image, pi_g; q2048_table_fold: the members of an orbit and their
 * order).  Arrived without an ABI bump, detected by its symbol.  For every occupied source row with key c and row Qc:
 *   NOT CANONICAL  canonical_key(c).key != c: the row is skipped and counted, no status bit is set -- unfolding it would
 *             let two source rows meet on one destination row.  (A table the folded kernels wrote holds none.)
 *   MEMBERS   image_h(c), h = 0..7, in ascending h; an h whose key equals that of a smaller h is left out (boards with a
 *             stabiliser have 4, 2 or 1 distinct images).
 *   FRAME     The inverse of the fold's.  A member m gets the row in ITS OWN frame, as the fused rollout reads it when
 *             it meets that board: Q_m[a] = Qc[pi_g(a)], g = the smallest g with image_g(m) = c.  Member h = 0 is c
 *             itself, with Qc unchanged.
 *   mode, w   Every member row finds or creates the row of m in `dst` and is combined with it exactly as
 *             q2048_table_merge combines a source row: its arithmetic (float32, every product and sum rounded on its
 *             own, 1 - w computed once on the host), its created-row rule (ADD creates w * q, the others q).
 *   counters  device uint64[6], ADDED to: [0] occupied src rows read, [1] src rows skipped as not canonical, [2] member
 *             rows produced, [3] rows created in dst, [4] rows combined with an existing dst row, [5] member rows
 *             dropped (no slot within the bulk probe limit); [2] = [3] + [4] + [5] = the sum of the distinct image
 *             counts of the canonical rows read.
 *   status    may be NULL; Q2048_STATUS_TABLE_FULL / Q2048_STATUS_DEEP_ROW as q2048_table_merge.
 * One streaming pass over `src` and up to eight find-or-creates in `dst` per occupied slot.  Distinct canonical keys
 * have disjoint orbits and one lane writes all members of its orbit, so exactly one lane writes each dst row: the only
 * races are the slot claims, the result depends on the two tables' ROWS only, and a float32 model on the host gives the
 * same bits.  Stream-ordered.  Nothing else may write `src` or touch `dst` while the call is in flight.  `src` is never
 * written; the `reserved` words of both tables are neither read nor written (line summaries in `src` are harmless, those
 * of `dst` are stale afterwards, as after a merge).  Keys salted by Q2048_FLAG_INDEPENDENT cannot be told from board
 * keys and must not be passed.
 * Errors, in the order of q2048_table_fold: dst, src or counters NULL -> Q2048_ERR_NULL; key_words == 2 ->
 * Q2048_ERR_UNSUPPORTED (5x5 has no folded table); key_words not 1 or 2, or a cap_log2 outside 4..40 -> Q2048_ERR_SIZE;
 * a table not 16-byte aligned -> Q2048_ERR_ALIGN; an unknown mode -> Q2048_ERR_FLAGS; w not finite, or outside [0, 1]
 * with Q2048_MERGE_BLEND -> Q2048_ERR_RANGE; the two tables' byte ranges overlap -> Q2048_ERR_RANGE. */
int q2048_table_unfold(q2048_slot *dst, int dst_cap_log2, const q2048_slot *src, int src_cap_log2, int key_words,
                       int mode, float w, uint64_t *counters, uint32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* Q2048_H */
