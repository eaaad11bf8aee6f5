/* colosseum_hip.h -- C ABI of libcolosseum_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary for the colosseumrl hot path: the batched equivalents of
 *   BaseEnvironment.new_state / next_state / valid_actions (+ the winners output)
 * for the Tron, TicTacToe and Blokus environments.  Plain pointers and sizes, no
 * torch types.  The reference's only native boundary is the Cython module
 *   colosseumrl/envs/tron/CyTronGrid.pyx:3-7   next_state_inplace(board, heads, directions, deaths, actions)
 *   colosseumrl/envs/tron/CyTronGrid.pyx:65    relative_player_inplace(board, num_players, player)
 * (C-contiguous buffers mutated in place, caller owns everything, no error path);
 * the entry points below keep those conventions and add what the Python layers
 * around it compute (rewards / terminal / winners, resets, legal-move sets).
 *
 * Conventions
 *   - every `void *`/typed pointer marked DEVICE is a device (HBM) address owned by the caller
 *     (the Python host passes torch-ROCm tensors' data_ptr()); kernels mutate state in place;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all calls are
 *     asynchronous on it, never synchronise the host, and are graph-capturable
 *     (crl_*_create / crl_destroy are the only calls that allocate or copy synchronously);
 *   - every function returns 0 on success and a negative CRL_E* code on error; nothing throws
 *     across the ABI; crl_last_error() returns a thread-local message for the last failure;
 *   - contexts are immutable after creation: any number of host threads may use one context
 *     concurrently on different buffers/streams (several env instances live under the GIL in
 *     the reference's MatchmakingServer.py:128-135);
 *   - env b of a batch of B owns board[b*cells .. (b+1)*cells) and element [p*B + b] of every
 *     per-player array ("[P][B]" struct-of-arrays: consecutive lanes touch consecutive bytes).
 *
 * There is NO CPU implementation behind this ABI.  The CPU restatement used by the tests lives
 * in oracle/ and is a different library.
 */
#ifndef COLOSSEUM_HIP_H
#define COLOSSEUM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRL_OK            0
#define CRL_EINVAL       -1   /* bad argument (null pointer, size out of range, ...) */
#define CRL_EHIP         -2   /* HIP runtime error (message has hipGetErrorString) */
#define CRL_ENODEV       -3   /* no gfx950 device visible */
#define CRL_EUNSUPPORTED -4

#define CRL_TRON_MAX_P   8
#define CRL_TTT_MAX_P    8
#define CRL_TTT_MAX_LINES 256

/* flags for *_step */
#define CRL_STEP_AUTO_RESET 1u  /* after writing the step outputs, reset every env that just became terminal */
/* crl_tron_step only, kept for existing callers: accepted and change nothing, crl_tron_step has one kernel (byte probes in
 * HBM; boards staged through LDS were slower on every shape measured and are gone) */
#define CRL_STEP_BYTES      2u
#define CRL_STEP_STAGED     4u
/* crl_blokus_step_single only: the learner's action is a RANK into its ordered legal list (as crl_blokus_select) */
#define CRL_STEP_RANK_ACTION 8u
/* flags for crl_tron_rollout */
#define CRL_ROLLOUT_NO_LDS  2u  /* force the lane-per-game global-memory kernel even when the boards would fit in LDS */
#define CRL_ROLLOUT_BYTES   4u  /* force the lane-per-game byte-per-cell LDS kernel */
#define CRL_ROLLOUT_BITS    8u  /* force the lane-per-game bitboard LDS kernel with replay epilogue (default for boards 21..40 wide with P > 4 and T >= 256) */
#define CRL_ROLLOUT_QUAD   16u  /* the lane-per-player kernel (four lanes per game): boards up to 20x20 with at most 4 players.
                                 * It is the default there; elsewhere the flag is ignored */
#define CRL_ROLLOUT_QBITS  32u  /* the lane-per-player bitboard kernel with replay epilogue (at most 4 players, boards up to
                                 * 40x40): the default for boards 21..40 wide in launches of more than 18 steps (shorter ones
                                 * stay in global memory: the kernel's fixed cost is worth that many steps there); with more
                                 * than 4 players the flag is ignored */

#define CRL_ROLLOUT_PAIR  128u  /* the byte-slab kernel with TWO lanes per game (boards up to 20x20, one or two players; elsewhere the
                                 * flag is ignored): the default there for launches of 32 steps and more (256 where a row is not whole dwords) */
#define CRL_ROLLOUT_GQUAD  64u  /* one lane per player on boards in GLOBAL memory (any board size, at most 4 players; with more
                                 * the flag is ignored): the default wherever the boards are not played out of LDS */

typedef struct crl_ctx crl_ctx;   /* opaque, immutable after creation */

const char *crl_last_error(void);
/* ABI revision of this header: bumped whenever a struct passed by value (crl_*_stats), an argument list or the RNG
 * contract of the sampled agents changes.  crl_version() returns the revision the LIBRARY was built from; a binding must
 * refuse a library whose revision differs from the header it was written against (colosseumrl_amd/_native.py does).
 * 100: round 1.  101: crl_tron_stats gained `packed`.  102: TicTacToe sampled agent draws 8 plies per Philox block.
 * 104: round 4.  105: crl_stream_wait_mapped.  106: crl_diag_issue_probe.  107: crl_blokus_fits.  108: crl_diag_bounds.
 * 109: crl_blokus_step / _step_observe place ANY action as the reference's next_state does (numpy index rules, extended ids,
 *      CRL_BLOKUS_*_ERROR codes in the reward slot).  110: crl_tron_next_state_inplace64 (+ _host) / _relative_player_inplace64.  111: crl_ttt_step_board_host.
 * 112: crl_tron_sample_avoid / crl_tron_rollout_avoid (the scripted avoid agent), crl_tron_step_single.
 * 113: crl_ttt_step_single / crl_blokus_step_single (one learner against the random agent), CRL_STEP_RANK_ACTION.
 *      crl_ttt_playout / crl_blokus_playout (batched random playouts) were added under 113: new entries and new Philox
 *      tags only, no existing struct, argument list or RNG contract changed.  So was crl_tron_playout (with
 *      CRL_PLAYOUT_AVOID / CRL_PLAYOUT_UNTIL_SEAT_DONE), on the same terms, and so were crl_tron_territory /
 *      crl_tron_sample_territory (Voronoi territory and the territory-greedy agent: two new entries, one new Philox tag).
 *      So were crl_ttt_winning_cells and crl_ttt_sample_tactical / _rollout_tactical / _step_single_tactical /
 *      _playout_tactical (the win-or-block agent of TicTacToe: five new entries, two new Philox tags), and
 *      crl_ttt_mcts / crl_ttt_mcts_max_simulations (batched tree search: two new entries, one new Philox tag), and
 *      crl_ttt_sample_mcts / _rollout_mcts / _step_single_mcts (the search as a seated agent: three new entries, no new tag), and
 *      crl_tron_mcts / crl_tron_mcts_max_simulations (batched tree search for one seat of Tron: two new entries, no new tag), and
 *      crl_tron_mcts_territory (that search with Voronoi territory at the leaves: one new entry, no new tag), and
 *      crl_tron_sample_mcts_territory / _max_simulations (that search as a seated agent: two new entries, no new tag), and
 *      crl_blokus_mcts / crl_blokus_mcts_max_simulations (tree search with progressive widening: two new entries, no new tag), and
 *      crl_ttt_puct_tree_bytes / _begin / _select / _backup / _root (tree search valued by the caller: five new entries, no new tag), and
 *      crl_tron_puct_tree_bytes / _begin / _select / _backup / _root (that search for one seat of Tron: five new entries, no new tag). */
#define CRL_ABI_VERSION 113
int crl_version(void);
/* number of visible HIP devices, or a negative code */
int crl_device_count(void);
void crl_destroy(crl_ctx *ctx);

/* ------------------------------------------------------------------ host staging for single-state callers
 * The reference's API is one state per call (BaseEnvironment.next_state, match_server.py:201-203): for such a caller a
 * hipMemcpy each way costs more than the step.  crl_host_alloc returns `bytes` of zeroed, page-locked host memory that
 * the GPU maps (hipHostMalloc, mapped + coherent): every entry point of this header accepts `*device` (+ offsets)
 * wherever it takes a DEVICE pointer, so a B = 1 call reads its state from and writes its results to host memory
 * directly -- no copy, one crl_stream_synchronize per call.  `device` may be NULL when the caller only needs `*host`
 * (both name the same bytes; under ROCm's unified addressing they are usually equal).
 * crl_stream_create gives a non-blocking stream of the current device, so that env instances on different host
 * threads (MatchmakingServer.py:128-135) do not wait for each other's work. */
int crl_host_alloc(size_t bytes, void **host, void **device);
int crl_host_free(void *host);
int crl_stream_create(void **stream);
/* Only for streams crl_stream_create returned, and only once NOTHING else refers to them: a stream that was handed to another
 * runtime object (e.g. wrapped as torch.cuda.ExternalStream, or with events / graphs of another library recorded on it) stays
 * referenced there, and destroying it under that object crashes the process at ITS next use of the handle, not inside this
 * library (seen in round 4: a segmentation fault at interpreter exit).  Let the other owner go first, or give it a stream it
 * owns itself and pass THAT stream's handle to the crl_* calls instead. */
int crl_stream_destroy(void *stream);
/* the blocking calls of the ABI besides create / destroy: */
int crl_stream_synchronize(void *stream);
/* ... and the same wait done on MAPPED MEMORY: a one-thread kernel is queued behind whatever `stream` holds and stores `seq`
 * (system-scope release) into a 32-bit word of crl_host_alloc memory -- `flag_device` / `flag_host` name that word from the
 * two sides --, and the host spins on the word.  For the short launch chains of a single-state caller this returns ~3.5 us
 * earlier than hipStreamSynchronize (9.7 against 13.2 us for launch + wait, tools/ubench/mailbox_rtt.hip).  Results the
 * chain wrote to mapped memory are visible when the call returns.  The caller uses a fresh `seq` per call (any value other
 * than the word's current one).  After `timeout_s` seconds without the flag the call falls back to hipStreamSynchronize and
 * reports what that reports (a faulted stream never delivers). */
int crl_stream_wait_mapped(void *stream, uint32_t *flag_device, const volatile uint32_t *flag_host, uint32_t seq, double timeout_s);

/* ------------------------------------------------------------------ diagnostics
 * How fast does THIS device, as it runs now, issue vector instructions?  `blocks` workgroups of 256 threads (4 waves: one
 * per SIMD of a CU) each run `iters` loop trips of 64 independent 32-bit integer VALU instructions; out (DEVICE, blocks x 256
 * dwords) keeps the work alive, clk (DEVICE, 2 x uint64) receives what wave 0 counted around its loop: shader-clock ticks
 * and 100 MHz wall-clock ticks (ratio x 100 = MHz under this load).  Asynchronous; time the launch with events: wave64
 * instructions per second = blocks x 4 x iters x 64 / time.  bench.py runs it at 4 waves per SIMD next to the rollouts, so
 * that a box whose clocks are capped shows in the record (the rollout kernels are bound by instruction issue). */
int crl_diag_issue_probe(uint32_t *out, uint64_t *clk, int blocks, int iters, void *stream);
/* The bounds asserts of a -DCRL_BOUNDS build (tools/gpu_bounds.sh; GPU AddressSanitizer is not available on the pool): out12
 * (HOST) = {failed checks, code of the first, its value, its limit} for tron.hip, ttt.hip and blokus.hip -- the range checks
 * on the kernels' data-dependent LDS / table accesses.  Synchronises the device.  Returns 1 from a build with the asserts
 * (after a self-test: a check that must fail is run and must be recorded), 0 from the shipped build, which compiles no
 * check and reports zeros; negative on error. */
int crl_diag_bounds(uint32_t *out12);

/* ------------------------------------------------------------------ RNG (exposed for parity tests) */
/* out[i*4..i*4+3] = Philox-4x32-10(ctr[i*4..], key); n counters; DEVICE pointers */
int crl_philox4x32(const uint32_t *ctr, uint32_t key0, uint32_t key1, uint32_t *out, int64_t n, void *stream);

/* ------------------------------------------------------------------ Tron
 * State (reference TronGridEnvironment.py:256-263, int64 there):
 *   board  int8  [B][N*N]   0 empty, p+1 = trail/head of player p
 *   heads  int16 [P][B]     flat y*N+x
 *   dirs   int8  [P][B]     0 N(y-1) 1 E(x+1) 2 S(y+1) 3 W(x-1)
 *   deaths int8  [P][B]     0 alive, else 1-based killer id
 */
/* replaces the per-instance set-up of TronGridEnvironment.__init__/generate_start_positions
 * (TronGridEnvironment.py:92-118,183-226); start_* are HOST arrays of length P */
int crl_tron_create(int N, int P, const int16_t *start_heads, const int8_t *start_dirs, crl_ctx **out);
/* Boards up to 20x20 with at most 4 players: crl_tron_create also builds, on the host, the table of per-lane constants of
 * the byte-slab lane-per-player rollout kernel (slab offsets of the rows a lane copies, its seat's start cell, its share of
 * the walls and of a rewritten row, the action table; layout: csrc/tron_lane_table.hpp).  The context owns it; the first
 * rollout on a device uploads it there once, crl_destroy frees every copy.  This call copies the HOST table out (for
 * tests): returns its length in dwords, or 0 for a context without one; table may be NULL, at most cap dwords are written. */
int crl_tron_lane_table(const crl_ctx *ctx, uint32_t *table, int cap);

/* replaces TronGridEnvironment.new_state (TronGridEnvironment.py:228-263) for B envs.
 * mask (DEVICE, uint8 [B]) may be NULL = reset all; else only envs with mask[b] != 0 */
int crl_tron_reset(const crl_ctx *ctx, int64_t B, const uint8_t *mask,
                   int8_t *board, int16_t *heads, int8_t *dirs, int8_t *deaths, void *stream);

/* replaces CyTronGrid.next_state_inplace (CyTronGrid.pyx:3-62) + the tail of
 * TronGridEnvironment.next_state (TronGridEnvironment.py:309-323) for B envs.
 *   actions  int8 [P][B] in {0 forward, +1 right, -1 left} (dead players' entries ignored; not validated, exactly
 *            like the reference's Cython kernel: other values are taken mod 4, so 2 would reverse)
 *   rewards  int8 [P][B] out: -1 dead, +1 alive, +10 surviving winner
 *   terminal uint8 [B]   out: alive <= 1
 *   winners  uint8 [B]   out: bitmask of alive players if terminal, else 0 (reference: None) */
int crl_tron_step(const crl_ctx *ctx, int64_t B,
                  int8_t *board, int16_t *heads, int8_t *dirs, int8_t *deaths,
                  const int8_t *actions, int8_t *rewards, uint8_t *terminal, uint8_t *winners,
                  uint32_t flags, void *stream);

/* per-env rollout bookkeeping, all DEVICE arrays (none may be NULL except `results`) */
typedef struct {
    uint32_t *tcount;       /* [B] rollout steps this env has taken so far = the RNG counter */
    uint32_t *tstep;        /* [B] steps taken in the current episode */
    uint32_t *n_episodes;   /* [B] episodes finished */
    uint32_t *win_count;    /* [P][B] */
    uint32_t *len_sum;      /* [B] */
    int32_t  *ret_sum;      /* [P][B] sum of rewards */
    uint8_t  *last_winners; /* [B] */
    uint16_t *last_len;     /* [B] */
    int32_t  *results;      /* [B][3+2P] or NULL: the per-game row the end-of-rollout gather ships, rewritten by every
                             * launch from the running totals above: n_episodes, len_sum, last_winners, win_count[P],
                             * ret_sum[P] (no separate packing pass over the SoA arrays) */
    uint16_t *packed;       /* [B][CRL_TRON_PACKED_ROW(P)] or NULL: the same row in 16-bit fields for a latency-bound
                             * gather (winners mask + episode length + P int16 returns; 16 bytes per game at
                             * P = 4 instead of 44): n_episodes, len_sum, last_winners, tstep (steps into the unfinished
                             * episode), ret_sum[P] as int16 -- the LOW 16 bits of the running totals, hence exact while
                             * the totals span at most 3,276 steps (|ret_sum| <= 10 per step); the host side ships this
                             * row only then (colosseumrl_amd/parallel.py) and the int32 row otherwise */
} crl_tron_stats;
#define CRL_TRON_PACKED_ROW(P) ((4 + (P) + 1) & ~1)   /* u16 entries per game: a whole number of dwords */

/* T fused env-steps per env with a uniform random agent and auto-reset (the benchmark loop of
 * BASELINE.md section 3; no reference counterpart -- the reference steps one env per Python call).
 * RNG contract, keyed by (seed, global env g = first_env_id + b, the env's step count c = tcount, player p);
 * one Philox call serves 8 consecutive steps of up to 4 players:
 *   W = Philox4x32-10(ctr = {g, c >> 3, p >> 2, 0x54520000}, key = {seed lo, seed hi})
 *   j = c & 7;  v = W[j >> 1] * 3^((j & 1) * 4 + (p & 3))  (mod 2^32)
 *   a = mulhi32(v, 3): 0 -> forward, 1 -> right, 2 -> left        (base-3 digits of the fraction W/2^32)
 * Boards up to 40x40 are played out of LDS (one copy in / one copy out per launch): boards up to 20x20 on a
 * byte-per-cell slab (one lane per player when P <= 4, else one lane per game), larger ones on an occupancy bitboard
 * (one lane per player when P <= 4; else one lane per game and T >= 256) whose unfinished episode is replayed with
 * owners at the end of the launch (P <= 4: by a second kernel queued behind the first).  Boards above 40x40 stay in global memory -- and so do, with P <= 4, launches too short
 * to earn an LDS kernel's copies back (one step on boards up to 20x20, up to 18 steps on boards 21..40 wide, 32 where a row
 * is not whole dwords): one lane per player (CRL_ROLLOUT_GQUAD; no fixed cost per launch) or one lane per game
 * (CRL_ROLLOUT_NO_LDS; episode tags, one pass over the boards per launch: P > 4, and launches on boards above 40x40 that are
 * long enough to earn that pass back -- from 15..57 steps on with one to three players, from 49..201 with four above 44x44).
 * CRL_ROLLOUT_BYTES / _BITS /
 * _QUAD / _QBITS pin one of the LDS kernels.  All give identical results.  The LDS kernels rely on the invariant of every state
 * produced by crl_tron_reset / crl_tron_step / crl_tron_rollout: board[heads[p]] == p + 1 for every player; callers
 * that upload hand-made states run crl_tron_check_state first (heads outside the board are clamped onto it, so a
 * broken state gives wrong results, never a wild access). */
int crl_tron_rollout(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T,
                     int8_t *board, int16_t *heads, int8_t *dirs, int8_t *deaths,
                     crl_tron_stats stats, uint32_t flags, void *stream);

/* crl_tron_rollout with HIP events ATTACHED TO THE DISPATCHES: start_event (hipEvent_t as void*, may be NULL) is updated
 * with the start of the rollout's first kernel, stop_event (may be NULL) with the end of its last one
 * (hipExtLaunchKernelGGL) -- the kernel time of a short launch without the marker packets and the ~3.6 us of host time
 * two hipEventRecord calls around it cost.  The events must have been created (and, for hipEventElapsedTime, are complete
 * once the stream is synchronised).  No reference counterpart. */
int crl_tron_rollout_timed(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T,
                           int8_t *board, int16_t *heads, int8_t *dirs, int8_t *deaths,
                           crl_tron_stats stats, uint32_t flags, void *stream, void *start_event, void *stop_event);

/* Counts (adds to *n_bad, a device int32 the caller zeroes) the games whose state breaks what every state produced by
 * crl_tron_reset / _step / _rollout satisfies and the LDS rollout kernels rely on: every head inside the board and
 * board[heads[p]] == p + 1.  For callers that upload hand-made states before a rollout.  No reference counterpart. */
int crl_tron_check_state(const crl_ctx *ctx, int64_t B, const int8_t *board, const int16_t *heads, int32_t *n_bad,
                         void *stream);

/* The random agent of crl_tron_rollout as a stand-alone call: actions[p*B+b] (0 forward, +1 right, -1 left, the
 * crl_tron_step encoding) of step tcount[b] of env first_env_id + b under the RNG contract above; advance != 0 also
 * increments tcount.  T x (crl_tron_sample; crl_tron_step with CRL_STEP_AUTO_RESET) leaves the same state as
 * crl_tron_rollout(T); callers overwrite the rows of the players they control.  No reference counterpart. */
int crl_tron_sample(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, uint32_t *tcount, int advance,
                    int8_t *actions, void *stream);

/* The reference's scripted opponent, SimpleAvoidAgent.__call__ (colosseumrl/envs/tron/rllib.py:68-95; the default opponent of
 * TronRaySinglePlayerEnvironment), for player p of global game g = first_env_id + b at step counter c = tcount[b].
 * Contract -- one Philox call per (game, step, player) under its own domain tag (the random agent's above is untouched):
 *   W = Philox4x32-10(ctr = {g, c, p, 0x54410000}, key = {seed lo, seed hi})
 *   noisy  iff  W[0] < thr,  thr = min(2^32, ceil(noise * 2^32)) computed on the host in 64 bits: noise = 0 is never noisy,
 *          noise = 1 always.  (The reference tests random.random() <= noise; the tie is an event of measure zero and is
 *          the one place where the two differ.)
 *   noisy:  a = mulhi32(W[1], 3): 0 forward, 1 right, 2 left  (the order of random.choice(['forward', 'right', 'left'])).
 *   else:   with `cell(dir)` = next_cell(x, y, dir, N) WITH clamping (TronGridEnvironment.py:467-481: a move off the board is
 *           clamped back onto it, so at a wall the cell ahead is the head itself, which is occupied):
 *           board[cell(d)] == 0                       -> forward;
 *           else side = W[2] >> 31: 0 = (+1, right, left), 1 = (-1, left, right); board[cell((d + offset) mod 4)] == 0 ->
 *           the first action of the pair, else the second.
 *   0 is "free" in the state and in every relabelled observation alike, so the agent reads the STATE board (no observation
 *   needed).  All players decide on the pre-step board (the reference computes every action before next_state).
 * crl_tron_sample_avoid writes actions[p*B+b] (0 forward, +1 right, -1 left, the crl_tron_step encoding; dead players: 0)
 * ONLY for the players whose bit is set in player_mask: the other rows are left untouched, so a caller writes its learner's
 * row and one launch fills in the opponents.  advance != 0 increments tcount, as crl_tron_sample does.  One lane per
 * (player, game): one Philox call and three byte probes (ahead, right, left) of the board.
 * Errors (CRL_EINVAL): noise outside [0, 1] or NaN, player_mask bits >= P, NULL pointers.  No reference counterpart
 * as a batched call. */
int crl_tron_sample_avoid(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, uint32_t *tcount, int advance,
                          double noise, uint32_t player_mask, const int8_t *board, const int16_t *heads, const int8_t *dirs,
                          const int8_t *deaths, int8_t *actions, void *stream);

/* T fused steps with EVERY player on the avoid agent, auto-reset, and the crl_tron_stats bookkeeping of crl_tron_rollout.
 * Bit-exact equivalent of
 *   T x (crl_tron_sample_avoid(all players, advance = 1); crl_tron_step(CRL_STEP_AUTO_RESET))
 * plus the statistics that loop implies (as crl_tron_rollout keeps them).  One launch (per 16,383 steps): with P <= 4 one lane
 * per player on boards in global memory (any board size; the quad shares the alive count and the reset), with P = 5..8 one
 * lane per game (same results).  Every step decides on the pre-step board before any lane of the game stores.  flags must
 * be 0 (reserved).  Argument checks as crl_tron_sample_avoid and crl_tron_rollout. */
int crl_tron_rollout_avoid(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T, double noise,
                           int8_t *board, int16_t *heads, int8_t *dirs, int8_t *deaths, crl_tron_stats stats, uint32_t flags,
                           void *stream);

/* One step of B "learner against scripted opponents" games (reference TronRaySinglePlayerEnvironment.step,
 * colosseumrl/envs/tron/rllib.py:131-153, batched): player 0 plays learner_action[b] (int64: 0 forward, 1 right, 2 left;
 * other values are taken mod 3), players 1..P-1 play rows 1..P-1 of actions (int8 [P][B], the crl_tron_step encoding; row 0
 * is not read -- fill the others with crl_tron_sample_avoid).  Outputs: reward int8 [B] = the learner's crl_tron_step reward,
 * terminal uint8 [B] = the game ended, done uint8 [B] = the learner died or the game ended; the done games are reset to the
 * start layout in the same launch (the state then is new_state's, as after CRL_STEP_AUTO_RESET).  Player 0's relative
 * observation IS the state (relabelling for player 0 is the identity).  One launch, one lane per game. */
int crl_tron_step_single(const crl_ctx *ctx, int64_t B, int8_t *board, int16_t *heads, int8_t *dirs, int8_t *deaths,
                         const int8_t *actions, const int64_t *learner_action, int8_t *reward, uint8_t *done, uint8_t *terminal,
                         void *stream);

/* ------------------------------------------------------------------ batched playouts (Tron)
 * crl_tron_playout: from each of B positions, play R games to their end for a seat and count the outcomes -- the
 * evaluation primitive of flat Monte Carlo (the Tron counterpart of crl_ttt_playout / crl_blokus_playout below).  One
 * launch, no host sync.
 * Inputs are read only: board / heads / dirs / deaths have crl_tron_step's layouts and are never written.  tcount uint32
 * [B] is the counter base (NULL means 0).  seat int8 [B] is the player evaluated (NULL means player 0, the learner of
 * TronSinglePlayerVectorEnv).  cand int32 [B][A] is the seat's first action in crl_tron_step_single's encoding (0 forward,
 * 1 right, 2 left); any other value (-1 padding included) skips its row.  cand == NULL requires A == 1: the position is then
 * evaluated as it stands (no forced first action, a = 0 below).
 * Playout r = 0 .. R-1 of row (b, a), on a private copy of position b: step k = 0, 1, ... has counter c = tcount[b] + k
 * (uint32).  At step 0 the seat plays cand[b][a] and uses no draw; every other player draws at c.  At every later step every
 * live player draws, the seat included.  Each step is exactly crl_tron_step without reset (the reference's sequential order
 * and head-on rule).  The playout stops after the first step crl_tron_step reports terminal (alive <= 1); with
 * CRL_PLAYOUT_UNTIL_SEAT_DONE also after the step in which the seat dies (crl_tron_step_single's `done`); with max_steps > 0
 * also after max_steps steps (0: no cap; every game ends within N*N steps).
 * Agent: the random agent; with CRL_PLAYOUT_AVOID the avoid agent with `noise` (all players decide on the pre-step board).
 * Random stream, g = low 32 bits of first_env_id + b, p the player:
 *   random  W = Philox4x32-10(ctr = {g, c >> 3, (a << 16) | r, 0x54700000 | (p >> 2)}, key = {seed lo, seed hi}), then
 *           crl_tron_rollout's digit rule with j = c & 7 and p & 3;
 *   avoid   W = Philox4x32-10(ctr = {g, c, (a << 16) | r, 0x54610000 | p}, key = {seed lo, seed hi}), then
 *           crl_tron_sample_avoid's rule (threshold, clamped probes, side bit).
 * The tags differ from every other stream's, so a playout never sees an env's real future draws.
 * Outputs, every row written (overwritten, never accumulated; a skipped row holds zeros):
 *   played  uint32 [B][A]     R, or 0 when the row is skipped;
 *   wins    uint32 [B][A][P]  playouts whose last step was terminal with bit p set in the winners mask (a capped or
 *                             seat-done stop that is not terminal counts for nobody);
 *   len_sum uint32 [B][A]     steps played, step 0 included;
 *   ret_sum int32  [B][A]     the seat's crl_tron_step rewards summed over the steps played (with UNTIL_SEAT_DONE: the
 *                             TronSinglePlayerVectorEnv episode return from that state and first action).
 * Every row of position b is skipped when the seat is outside [0, P), the seat is dead (deaths[seat][b] != 0), or P >= 2 and
 * fewer than two players are alive.  With P = 1 every playout is one terminal step.
 * Argument checks (CRL_EINVAL, with a crl_last_error message, before any device work): NULL state / output pointers, B out
 * of range, R or A outside [1, 65535], A != 1 with cand == NULL, noise outside [0, 1] or NaN, max_steps outside [0, 65535],
 * flags other than the two below.  Lanes are indexed with 64-bit arithmetic: B * A * R may pass 2^31.
 * Precondition: crl_tron_check_state's invariant, cells holding 0..P; a broken state gives wrong results, never a wild
 * access.  One lane per playout on a private occupancy bitboard in LDS (a cell is occupied iff its value is > 0; the owner
 * of a hit head is the player whose head is there); outcomes are summed per row inside the wave (shuffles) before one store
 * or integer atomic per row segment and output word, so the results do not depend on the order of the waves. */
#define CRL_PLAYOUT_AVOID           1u   /* crl_tron_playout: every player on the avoid agent (default: the random agent) */
#define CRL_PLAYOUT_UNTIL_SEAT_DONE 2u   /* crl_tron_playout: also stop after the step in which the seat dies */
int crl_tron_playout(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                     const int8_t *board, const int16_t *heads, const int8_t *dirs, const int8_t *deaths,
                     const uint32_t *tcount, const int8_t *seat, const int32_t *cand, int A, int R,
                     double noise, int max_steps,
                     uint32_t *wins, uint32_t *played, uint32_t *len_sum, int32_t *ret_sum,
                     uint32_t flags, void *stream);

/* ------------------------------------------------------------------ batched tree search for a seat (UCT), Tron
 * crl_tron_mcts: from each of B positions build a search tree of its own for ONE seat by S simulations s = 0 .. S-1, in
 * order, each evaluated by R playouts, and report the root's children.  One launch, no host sync.  Added under revision 113:
 * two new entries, no new Philox tag, no existing struct, argument list or RNG contract changed.
 * The search is single-agent: the tree branches on the seat's three actions only.  Every other player is part of the
 * transition, played by a scripted MODEL (the random or the avoid agent) from counter-based draws, so a node's position is a
 * pure function of the root and the edge sequence.
 * State.  Read only, in crl_tron_playout's layouts: board / heads / dirs / deaths as crl_tron_step has them, tcount uint32 [B]
 * the counter base (NULL means 0), seat int8 [B] the player searched for (NULL means player 0).  g = the low 32 bits of
 * first_env_id + b.  A cell is occupied iff its value is > 0.
 * Flags.  CRL_PLAYOUT_AVOID only: the model and the playouts then use the avoid agent with `noise`, else the random agent
 * (noise is checked and otherwise unused).
 * Nodes.  Node 0 is the root, position b.  A node holds n, the number of simulations that passed through it; w, the seat's
 * half-points summed over them (the root's w stays 0); and three child slots, for the actions 0 forward, 1 right, 2 left
 * (crl_tron_step_single's encoding), all empty at first.
 * A tree step from a node at depth k (edges from the root) with edge action e has step counter c = tcount[b] + k (uint32
 * arithmetic).  The seat plays e.  Every other live player q plays the model agent, decided on the pre-step position:
 *   random  W = Philox4x32-10(ctr = {g, c >> 3, 0xFFFF0000, 0x54700000 | (q >> 2)}, key = {seed lo, seed hi}), then
 *           crl_tron_rollout's digit rule with j = c & 7 and q & 3;
 *   avoid   W = Philox4x32-10(ctr = {g, c, 0xFFFF0000, 0x54610000 | q}, key = {seed lo, seed hi}), then
 *           crl_tron_sample_avoid's rule (threshold, clamped probes, side bit).
 * The step itself is crl_tron_step without reset.  These are the two playout tags; crl_tron_playout has a < 65535 and the
 * leaves below have s <= 4094, so the third word 0xFFFF0000 belongs to the tree steps alone.  The node reached is CLOSED iff
 * the seat is dead or at most one player is alive; a closed node's outcome is 2 half-points iff the seat is alive, else 0.
 * Descent, as crl_ttt_mcts's.  A simulation starts at the root with a private copy of the position.  At an open node v:
 *   expand: if some action has no child, take the lowest such action e; a new node with the next free index becomes v's
 *           child at e, the tree step e is played, and the new node is the leaf, closed or not;
 *   select: else take the child u that maximises score(v, u), ties to the lowest action, and play its tree step; a closed
 *           child is the leaf, else the descent continues at u.
 * Score, crl_ttt_mcts's, in 64-bit integers with floor divisions:
 *   exploit = (w_u << 15) / (n_u * R)                                        in [0, 65536]
 *   lg(n), n >= 1: m = the index of n's leading one, f = ((n << (31 - m)) >> 23) & 255, lg(n) = 256 m + f
 *   X = (lg(n_v) << 24) / n_u
 *   score = exploit + ((cexp * isqrt(X)) >> 8),  isqrt the exact floor square root
 * (cexp / 256 multiplies sqrt(log2 n_v / n_u) on a value scale of 0 .. 1: 256 is the usual choice, 0 pure exploitation).
 * Evaluation of the leaf L at depth d.  Closed: all R playouts have L's outcome and no draw is made.  Open: playouts
 * r = 0 .. R-1, each crl_tron_playout's playout from L's position as it stands (cand == NULL there: no forced action), with
 * the counter base tcount[b] + d, the third counter word (s << 16) | r, the flag's agent and `noise`; it stops after the
 * first terminal step, after the step in which the seat dies (CRL_PLAYOUT_UNTIL_SEAT_DONE's rule), or after max_steps
 * playout steps when max_steps > 0.  Half-points of a playout: 2 if its last step was terminal with the seat in the winners
 * mask; 1 if the cap stopped it (the step was not terminal) with the seat alive; else 0.
 * Backup.  n += 1 on every node of the path from the root to L; w += the sum of the playouts' half-points on every node of
 * it but the root.
 * Outputs, every word overwritten:
 *   visits uint32 [B][3], value uint32 [B][3]   n and w of the root's child at each action, 0 where there is none;
 *   nodes  uint32 [B]                           the node count, root included;
 *   best   int32  [B]                           the most visited action; ties go to the larger w, then to the lower action.
 * A position is skipped (zeros, nodes 0, best -1) when the seat is outside [0, P), the seat is dead (deaths[seat][b] != 0),
 * or P >= 2 and fewer than two players are alive.
 * Limits (CRL_EINVAL, with a crl_last_error message, before any device work): NULL state or output pointers, B out of range
 * (as crl_tron_playout), S outside [1, S_max], R outside [1, 1024], cexp > 65535, noise outside [0, 1] or NaN, max_steps
 * outside [0, 65535], flags other than CRL_PLAYOUT_AVOID, a context that is not a Tron context.
 * S_max = min(4095, (65536 - 264 * ceil(N*N / 32)) / 16 - 1): one wave's tree and path (16 bytes per node) and its 66
 * occupancy bitboards (root, working copy, 64 playouts) fit 64 KB of one workgroup's LDS, and s fits its counter word --
 * 4,078 on 5x5, 3,897 on 19x19, 3,880 on 20x20, 3,270 on 40x40, 1,983 on 64x64.  Boards of 90x90 and more leave no room
 * (S_max < 1): both entries answer CRL_EUNSUPPORTED there.  crl_tron_mcts_max_simulations returns S_max of the context
 * (CRL_EINVAL on a context that is not a Tron context).
 * Precondition as crl_tron_playout: heads outside the board are clamped onto it (wrong results, never a wild access).
 * One wave per tree, the tree in LDS, one to four waves per workgroup; the descent is wave-uniform, lanes 0..2 score the
 * children, lane r plays playout r on a private bitboard (R > 64 in passes), lane i backs up the node at depth i.  Nothing is
 * shared between waves, so the results do not depend on their order.  Games are walked in a grid-stride loop with 64-bit
 * indices. */
int crl_tron_mcts_max_simulations(const crl_ctx *ctx);
int crl_tron_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                  const int8_t *board, const int16_t *heads, const int8_t *dirs, const int8_t *deaths,
                  const uint32_t *tcount, const int8_t *seat,
                  int S, int R, uint32_t cexp, double noise, int max_steps,
                  uint32_t *visits, uint32_t *value, uint32_t *nodes, int32_t *best,
                  uint32_t flags, void *stream);
/* crl_tron_mcts_territory: crl_tron_mcts with Voronoi territory as the leaf evaluator -- a leaf is valued by ONE flood of its
 * position, there are no playouts, and nothing is drawn at a leaf.  One launch, no host sync.  Added under revision 113: one
 * new entry, no new Philox tag, no existing struct, argument list or RNG contract changed.
 * Unchanged from crl_tron_mcts, word for word: the state layouts and the read-only state; g; the NULL rules of tcount and
 * seat; nodes and child slots; the tree step at depth k (the seat plays e, every other live player the model agent -- the
 * random agent, or with CRL_PLAYOUT_AVOID the avoid agent with `noise` -- from the two playout tags under the third counter
 * word 0xFFFF0000 at counter tcount[b] + k); the CLOSED rule; expand / select with ties to the lowest action; the integer
 * score with its lg, floor divisions and exact isqrt; backup; the four outputs and best's tie rule; the skipped-position rule
 * (zeros, nodes 0, best -1).
 * The differences.  V in [1, 1024] is the value scale and stands wherever R stands in crl_tron_mcts:
 *   exploit = (w_u << 15) / (n_u * V),
 * and a closed leaf is worth 2 V half-points iff the seat is alive, else 0.  There is no R, no max_steps and no draw at a
 * leaf.  An OPEN leaf L is valued by one Voronoi flood of its position:
 *   occupancy   the root's (a cell is occupied iff its board value is > 0, crl_tron_mcts's rule) plus every cell the tree
 *               steps on the path moved a head onto; a cell is FREE iff it is not occupied in that sense;
 *   players     LIVE, heads and directions are L's;
 *   area[p]     crl_tron_territory's definition (below) on that position with nobody forced (its cand == NULL case): the
 *               first cells forward / right / left that are on the board and free, d_p, strict first arrival, ties belong
 *               to nobody, dead players get 0;
 *   a_s = area[seat], a_o = the maximum of area[q] over the other live players q (0 if there is none);
 *   half-points = (a_s + a_o == 0) ? V : floor(2 * V * a_s / (a_s + a_o)),  an integer in [0, 2 V].
 * An even split gives V, a seat with no territory 0, P = 1 with room 2 V.  Nothing overflows: 2 * 1024 * 4096 < 2^32, and a
 * node's w stays below 2^32 with n <= 4095.
 * Flags.  CRL_PLAYOUT_AVOID only; it selects the model agent of the tree steps.  noise is checked always and used only then.
 * Limits (CRL_EINVAL, with a crl_last_error message naming the argument, before any device work): NULL state or output
 * pointers, B out of range (as crl_tron_mcts), S outside [1, S_max], V outside [1, 1024], cexp > 65535, noise outside [0, 1]
 * or NaN, flags other than CRL_PLAYOUT_AVOID, a context that is not a Tron context.  S_max is crl_tron_mcts's
 * (crl_tron_mcts_max_simulations), unchanged, so that trees of the two searches compare at any S -- although a wave here needs
 * only 16 (S + 1) + 8 ceil(N*N / 32) bytes of LDS (the tree, the path, the root and the working bitboard; no playout slabs).
 * Boards wider than 64 answer CRL_EUNSUPPORTED: the flood runs inside the wave with one lane per board row.  Widths 65..89,
 * which crl_tron_mcts takes, are deliberately left out.
 * One wave per tree in crl_tron_mcts's mapping, one to four waves per workgroup (as many as fit 64 KB: four up to S = 1,017
 * on 19x19, 998 on 40x40, 959 on 64x64).  At an open leaf lane y < N is board row y: it cuts its row out of the working bitboard, builds the live
 * players' first cells in it, and the wave floods as the register kernels of crl_tron_territory do (32-bit rows up to
 * N = 32, 64-bit rows above). */
int crl_tron_mcts_territory(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                            const int8_t *board, const int16_t *heads, const int8_t *dirs, const int8_t *deaths,
                            const uint32_t *tcount, const int8_t *seat,
                            int S, int V, uint32_t cexp, double noise,
                            uint32_t *visits, uint32_t *value, uint32_t *nodes, int32_t *best,
                            uint32_t flags, void *stream);
/* crl_tron_sample_mcts_territory: the search of crl_tron_mcts_territory as a SEATED agent -- one action for every masked player
 * of every game, one launch, no host sync.  Added under revision 113: two new entries, no new Philox tag, no existing struct,
 * argument list or RNG contract changed.  The contract is made of two that exist.
 * crl_tron_sample_territory's (below), word for word: player_mask (rows outside it are never written), advance (!= 0
 * increments tcount[b], once per game whatever the mask), actions[p*B+b] in the crl_tron_step encoding (0, +1, -1), dead
 * players get 0, g = the low 32 bits of first_env_id + b and c = tcount[b].  The state is read only.
 * For a live masked player p:
 *   W = Philox4x32-10(ctr = {g, c, p, 0x54760000}, key = {seed lo, seed hi})      (crl_tron_sample_territory's own draw)
 *   noisy  iff  W[0] < thr(noise), thr as crl_tron_sample_avoid's;  noisy: a = mulhi32(W[1], 3): 0 forward, 1 right, 2 left
 *          -- so at noise = 1 the call returns exactly what crl_tron_sample_territory returns at noise = 1;
 *   else:  a = `best` of crl_tron_mcts_territory on the same state with seat = p, the same seed, first_env_id, tcount, S, V,
 *          cexp and flags, and model_noise as its `noise`; best = -1 (fewer than two players alive with P >= 2) plays 0.
 * All players decide on the pre-step state, and every search of game b reads tcount[b] before the call advances it.
 * Limits (CRL_EINVAL, with a crl_last_error message naming the argument, before any device work): NULL pointers (tcount and
 * actions included), B out of range (as crl_tron_mcts), player_mask zero or with bits >= P, noise or model_noise outside
 * [0, 1] or NaN, S outside [1, S_agent], V outside [1, 1024], cexp > 65535, flags other than CRL_PLAYOUT_AVOID, a context that
 * is not a Tron context.  With m = popcount(player_mask) and nwords = ceil(N*N / 32),
 *   S_agent(N, m) = min(S_max of crl_tron_mcts, floor((floor(65536 / m) - 8 nwords) / 16) - 1):
 * m waves of crl_tron_mcts_territory's per-wave LDS (16 (S + 1) + 8 nwords bytes) in one 64 KB workgroup -- 1,358 on 19x19
 * with m = 3, 447 on 64x64 with m = 8.  crl_tron_sample_mcts_territory_max_simulations returns S_agent of the context and the
 * mask (CRL_EINVAL on a context that is not a Tron context or a bad mask).  Boards wider than 64 answer CRL_EUNSUPPORTED in
 * both entries, as crl_tron_mcts_territory does.
 * One workgroup per game, wave j the j-th masked player with a tree of its own in its own slice of LDS (64 m threads); the
 * noise draw is wave-uniform and comes first, a noisy wave or a dead seat skips the search.  Every wave reads the counter,
 * then comes the one workgroup barrier of a game, then wave 0 stores c + 1.  Games are walked in a grid-stride loop with
 * 64-bit indices. */
int crl_tron_sample_mcts_territory_max_simulations(const crl_ctx *ctx, uint32_t player_mask);
int crl_tron_sample_mcts_territory(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                                   uint32_t *tcount, int advance, double noise, uint32_t player_mask,
                                   const int8_t *board, const int16_t *heads, const int8_t *dirs, const int8_t *deaths,
                                   int S, int V, uint32_t cexp, double model_noise, uint32_t flags,
                                   int8_t *actions, void *stream);

/* ------------------------------------------------------------------ Voronoi territory (Tron)
 * crl_tron_territory: for each of B positions and A forced first actions of a seat, the number of free cells every player
 * reaches strictly before every other player -- Tron's deterministic evaluator, an evaluation primitive beside
 * crl_tron_playout that needs no playouts.  One launch, no host sync.  No reference counterpart.
 * Definitions.  A cell is FREE iff its board value is 0; player p is LIVE iff deaths[p] == 0.  For a live player p the FIRST
 * CELLS F_p are the cells the actions forward / right / left lead to from (heads[p], dirs[p]) -- directions as in
 * CyTronGrid.pyx: 0 up, 1 right, 2 down, 3 left, a right turn is +1 mod 4 --, keeping those that are on the board and
 * free.  The cell behind the head is never a first cell, even where it is free (it is at the start layout).
 * Row (b, a) with a forced candidate cand[b][a] in {0 forward, 1 right, 2 left} (crl_tron_playout's encoding): the seat's
 * F is only that action's cell, and empty when that cell is off the board or occupied -- the row is then FATAL for the seat.
 *   d_p(c)        = 1 + the length of the shortest 4-connected path through free cells from any cell of F_p to the free
 *                   cell c; infinite if there is none.
 *   area[b][a][p] = the number of free cells c with d_p(c) finite and d_p(c) < d_q(c) for every other live q.
 * Dead players get 0.  A cell reached first by two or more players at the same distance belongs to nobody.
 * Inputs are read only: board / heads / dirs / deaths have crl_tron_step's layouts.  seat int8 [B] is the player forced
 * (NULL means player 0); cand int32 [B][A].  cand == NULL requires A == 1: nobody is forced and seat is not read.
 * Outputs, every row overwritten (never accumulated):
 *   area int32 [B][A][P]   (the layout of crl_tron_playout's wins);
 *   info uint8 [B][A]      bit 0: the row was evaluated; bit 1: the seat's forced cell is off the board or occupied.
 * A row is skipped (zeros, info 0) when a candidate is given and the seat is outside [0, P), the seat is dead, or the
 * candidate is outside 0..2 (-1 padding included).  A position with one live player or none is still evaluated: the area
 * is then that player's reachable cells.
 * Argument checks (CRL_EINVAL, with a crl_last_error message, before any device work): NULL state / output pointers, B out
 * of range, A outside [1, 16], A != 1 with cand == NULL, a context that is not a Tron context.  Rows are indexed with 64-bit
 * arithmetic.  Precondition as crl_tron_playout: heads outside the board are clamped onto it (wrong results, never a
 * wild access).
 * Method: a level-synchronous multi-source flood on occupancy bitboards; per level and live player new_p = expand(front_p)
 * & free, cells in two or more new_p are contested, area_p += popcount(new_p & ~contested), then free &= ~(union of new_p)
 * and front_p = new_p (contested cells stay in the frontiers: ties propagate).  Flooding only through cells nobody has
 * claimed is exact: a player arriving at a claimed cell later can neither win nor tie anything beyond it.  A flood ends when
 * a level adds no cell, and in any case after N*N levels.  Boards up to 64x64: one lane per board row (a 32- or 64-bit
 * word), floor(64 / N) rows (b, a) per wave, vertical neighbours by DPP wave shifts, frontiers and sums in registers.
 * Boards 65..181 wide: one workgroup per row (b, a), bitboards in LDS. */
int crl_tron_territory(const crl_ctx *ctx, int64_t B, const int8_t *board, const int16_t *heads, const int8_t *dirs,
                       const int8_t *deaths, const int8_t *seat, const int32_t *cand, int A, int32_t *area, uint8_t *info,
                       void *stream);

/* The territory-greedy scripted agent: crl_tron_sample_avoid's argument list and its player_mask / advance / actions
 * semantics (rows outside the mask are not written, dead players get 0, advance != 0 increments tcount; the same checks).
 * For each live masked player p of global game g = first_env_id + b at step counter c = tcount[b]:
 *   W = Philox4x32-10(ctr = {g, c, p, 0x54760000}, key = {seed lo, seed hi})            (a domain tag of its own)
 *   noisy  iff  W[0] < thr, thr as crl_tron_sample_avoid's;  noisy: a = mulhi32(W[1], 3): 0 forward, 1 right, 2 left;
 *   else:  the three candidates a = 0, 1, 2 are evaluated as crl_tron_territory rows with seat = p:
 *          score_a = area[p] - max over the other live q of area[q]  (no other live player: area[p]); a fatal candidate
 *          scores below every non-fatal one; the best score plays, ties go to the lowest index (forward, right, left).
 * All players decide on the pre-step board.  actions[p*B+b] in the crl_tron_step encoding (0, +1, -1).  One launch: one
 * wave (boards above 64x64: one workgroup) per game floods its 3 x (masked players) candidates. */
int crl_tron_sample_territory(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, uint32_t *tcount, int advance,
                              double noise, uint32_t player_mask, const int8_t *board, const int16_t *heads, const int8_t *dirs,
                              const int8_t *deaths, int8_t *actions, void *stream);

/* replaces CyTronGrid.relative_player_inplace (CyTronGrid.pyx:65-71) + the rolls of
 * TronGridEnvironment.state_to_observation (TronGridEnvironment.py:385-405), fully observable branch.
 * player int8 [B]: observer of env b.  ANY id is an observer, as in the reference (ABI 109): the rolled vectors use numpy's
 * modulo ((arange + player) % P, :393), the board C's remainder (CyTronGrid.pyx:1 cdivision=True) -- ids -128..P observe as
 * player mod P, beyond P low trail ids come out <= 0 exactly as there.  Outputs have the shapes of the state arrays. */
int crl_tron_observe(const crl_ctx *ctx, int64_t B, const int8_t *board, const int16_t *heads,
                     const int8_t *dirs, const int8_t *deaths, const int8_t *player,
                     int8_t *obs_board, int16_t *obs_heads, int8_t *obs_dirs, int8_t *obs_deaths, void *stream);

/* The same observation for ALL P observers in one pass (what a self-play learner consumes every step):
 * obs_board int8 [P][B][N*N], obs_heads int16 [P][P][B], obs_dirs / obs_deaths int8 [P][P][B]; slice [p] equals
 * crl_tron_observe with player[b] = p.  Streams N*N bytes in and P*N*N bytes out per game. */
int crl_tron_observe_all(const crl_ctx *ctx, int64_t B, const int8_t *board, const int16_t *heads, const int8_t *dirs,
                         const int8_t *deaths, int8_t *obs_board, int16_t *obs_heads, int8_t *obs_dirs, int8_t *obs_deaths,
                         void *stream);

/* One launch for what a self-play learner does every step: [sample ->] next_state -> state_to_observation of every
 * player, i.e. TronGridEnvironment.next_state (TronGridEnvironment.py:265-323, called per tick from match_server.py:201-203)
 * followed by state_to_observation (:363-420, match_server.py:218) for all P observers.  Exactly equivalent to
 *   [crl_tron_sample(..., advance = 1);]  crl_tron_step(..., flags);  crl_tron_observe_all(...)
 * with actions == NULL meaning "draw them with the rollout's random agent at tcount[b] and advance tcount" (tcount may be
 * NULL when actions are given; it is not touched then).  The boards are read from HBM once (coalesced, into LDS),
 * stepped there, and the P relabelled copies streamed out: N*N bytes in + P*N*N bytes out per game.  Boards with
 * N*N % 16 != 0 (the reference's default 19x19 among them) take the same route as one flat byte stream per workgroup when the
 * batch is a multiple of 16 games and the board buffers are 16-byte aligned; other batches of such boards, P = 8, or boards too
 * large for 16 LDS slabs take a kernel with one game per workgroup and byte accesses: still one launch, same results,
 * actions == NULL allowed. */
int crl_tron_step_observe(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                          int8_t *board, int16_t *heads, int8_t *dirs, int8_t *deaths,
                          const int8_t *actions, uint32_t *tcount,
                          int8_t *rewards, uint8_t *terminal, uint8_t *winners,
                          int8_t *obs_board, int16_t *obs_heads, int8_t *obs_dirs, int8_t *obs_deaths,
                          uint32_t flags, void *stream);

/* The Cython module's OWN functions with their own types (the reference's only native boundary), for callers that hold
 * reference states:
 *   CyTronGrid.pyx:3-7   next_state_inplace(long[:, ::1] board, long[::1] heads, long[::1] directions, long[::1] deaths,
 *                                           const long[::1] actions)
 *   CyTronGrid.pyx:65    relative_player_inplace(long[:, ::1] board, const long num_players, const long player)
 * int64, C-contiguous, the reference's layout (board [N][N]; heads / directions / deaths / actions [P]; actions in
 * {0 forward, +1 right, -1 left}), MUTATED IN PLACE, caller owns every buffer, no error path for the contents (as there).
 * The direction is computed as there, (directions[i] + action + 4) % 4 with C's remainder: sums below -4 give a negative
 * direction, the player then runs into the cell it stands on and the negative direction is stored -- 240 direct calls of the
 * reference function with such arguments are a golden fixture (values are read as 32-bit integers; heads must lie on the board).  B games lie one behind the other ([B][N*N], [B][P]); the
 * single-state drop-in class calls it with B = 1 on crl_host_alloc memory, so TronGridEnvironment.next_state neither
 * converts its four arrays to the batched steppers' int8 / int16 struct-of-arrays nor back.  The step touches the board where the
 * reference does: <= P probes, <= P trail stores.  Optional outputs (NULL to skip), what TronGridEnvironment.next_state
 * computes around the call (TronGridEnvironment.py:309-321): rewards int64 [B][P] (-1 dead, +1 alive, +10 surviving
 * winner), terminal uint8 [B], winners uint8 [B] (bitmask of the alive players if terminal, else 0).  Optional
 * observations of the NEW state for all P observers (all four pointers or none; TronGridEnvironment.py:385-405):
 * obs_board int64 [B][P][N*N] (relative_player_inplace of a copy with player = p + 1), obs_heads / obs_directions /
 * obs_deaths int64 [B][P][P] (rolled so index 0 is the observer). */
int crl_tron_next_state_inplace64(const crl_ctx *ctx, int64_t B, int64_t *board, int64_t *heads, int64_t *directions,
                                  int64_t *deaths, const int64_t *actions, int64_t *rewards, uint8_t *terminal, uint8_t *winners,
                                  int64_t *obs_board, int64_t *obs_heads, int64_t *obs_directions, int64_t *obs_deaths, void *stream);
/* The single-state form of the call above, ONE BLOCKING call for a caller whose state lies in crl_host_alloc memory (B = 1;
 * every pointer is such memory, which host and GPU address alike under ROCm's unified addressing -- a binding checks that
 * crl_host_alloc returned equal host / device addresses before it uses this entry): launch + completion.  Because the host can
 * read the state, the player vectors (heads, directions, deaths, actions) travel BY VALUE in the kernel arguments -- the
 * kernel's first data access is then the board probe, one PCIe round trip instead of two -- and the kernel publishes
 * completion itself: `seq` into *flag (a 32-bit word of crl_host_alloc memory; a fresh value per call) behind its last
 * store, on which the host spins (timeout_s and the fallback as crl_stream_wait_mapped).  No signal kernel, one call through
 * the binding instead of two.  Results as above, visible when the call returns. */
int crl_tron_next_state_inplace64_host(const crl_ctx *ctx, int64_t *board, int64_t *heads, int64_t *directions,
                                       int64_t *deaths, const int64_t *actions, int64_t *rewards, uint8_t *terminal, uint8_t *winners,
                                       int64_t *obs_board, int64_t *obs_heads, int64_t *obs_directions, int64_t *obs_deaths, void *stream,
                                       uint32_t *flag, uint32_t seq, double timeout_s);
/* board[b][i][j] > 0  ->  ((board - player[b] + num_players) % num_players) + 1 with C's remainder (cdivision=True), in place;
 * player int64 [B] as the reference passes it (TronGridEnvironment.py:390: the observer's id + 1). */
int crl_tron_relative_player_inplace64(const crl_ctx *ctx, int64_t B, int64_t *board, int64_t num_players, const int64_t *player,
                                       void *stream);

/* replaces TronGridEnvironment.compute_ranking (TronGridEnvironment.py:483-508) for B games:
 * rank int8 [P][B], 0 = best; trail-length scores, the mutual-kill tie rule (with its deaths[-1] read for
 * alive players) and competition ranking, exactly as the reference computes them */
int crl_tron_ranking(const crl_ctx *ctx, int64_t B, const int8_t *board, const int8_t *deaths, int8_t *rank, void *stream);

/* ------------------------------------------------------------------ TicTacToe (D0 x D1 x D2, K in a row, P players)
 * State (reference tictactoe_2p_env.py:165-169: (board int8, winner)):
 *   occ     uint32 [P][B]  bit c set = flat cell c (row-major) holds player p's mark
 *   winner  int8   [B]     -1 = None (sticky once set)
 *   to_move int8   [B]
 * For boards of at most 16 cells (the reference's 3x3 and 3x5) crl_ttt_create also puts an 8 KB table of the winning masks
 * on the device that is current at the call; crl_ttt_rollout uses it when it runs on that device (and computes the win test
 * as everywhere else when it does not, or when no device was there at create time; the environment variable
 * CRL_TTT_NO_WIN_TABLE, read by crl_ttt_create, skips the table: tests of that path).  crl_destroy frees it.
 */
int crl_ttt_create(int D0, int D1, int D2, int K, int P, crl_ctx **out);
/* number of win lines and a HOST copy of them (for tests); lines may be NULL */
int crl_ttt_lines(const crl_ctx *ctx, uint32_t *lines, int cap);
int crl_ttt_reset(const crl_ctx *ctx, int64_t B, const uint8_t *mask,
                  uint32_t *occ, int8_t *winner, int8_t *to_move, void *stream);
/* replaces TicTacToe{2,3,4}PlayerEnv.next_state (tictactoe_2p_env.py:240-315).
 *   action int8 [B]: flat cell index, or -1 for '' ; an occupied cell is a no-op that still passes the turn
 *   reward int8 [B] (the mover's), terminal uint8 [B], winners int8 [B] (-1 = None, else the winner) */
int crl_ttt_step(const crl_ctx *ctx, int64_t B, uint32_t *occ, int8_t *winner, int8_t *to_move,
                 const int8_t *action, int8_t *reward, uint8_t *terminal, int8_t *winners,
                 uint32_t flags, void *stream);
/* replaces TicTacToe*.valid_actions (tictactoe_2p_env.py:317-348): empties bitmask uint32 [B] */
int crl_ttt_valid(const crl_ctx *ctx, int64_t B, const uint32_t *occ, uint32_t *valid, void *stream);
/* int8 [B][cells] board (4-byte aligned) in the reference encoding (-1 empty), relative to `player` when player != NULL
 * (reference _relative_player_id, tictactoe_2p_env.py:26-27, modulus given by rel_mod) */
int crl_ttt_board(const crl_ctx *ctx, int64_t B, const uint32_t *occ, const int8_t *player, int rel_mod,
                  int8_t *board, void *stream);
/* One launch for a ply of every game, as a learner / vector env needs it: [sample ->] next_state -> valid_actions and
 * state_to_observation of the player to move NEXT.  Exactly equivalent to
 *   [crl_ttt_sample(..., advance = 1);]  crl_ttt_step(..., flags);  crl_ttt_valid(...);  crl_ttt_board(..., player = to_move, rel_mod)
 * with action == NULL meaning "draw it with the rollout's random agent at tcount[b] and advance tcount" (tcount may be NULL
 * when actions are given).  obs_board int8 [B][cells] (4-byte aligned), valid uint32 [B]. */
int crl_ttt_step_observe(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                         uint32_t *occ, int8_t *winner, int8_t *to_move, const int8_t *action, uint32_t *tcount,
                         int8_t *reward, uint8_t *terminal, int8_t *winners, int8_t *obs_board, uint32_t *valid,
                         int rel_mod, uint32_t flags, void *stream);
/* The same calls on states in the REFERENCE's own layout (tictactoe_2p_env.py:165-169): board int8 [B][cells], -1 = empty,
 * else the owner's id; winner / to_move as above.  For callers that hold reference states (the single-state drop-in
 * classes, on crl_host_alloc memory: one launch per next_state) and never see the occupancy masks.
 * crl_ttt_step_board == crl_ttt_step on the equivalent masks, the board updated in place (the one cell the move filled;
 * all -1 after an auto-reset), plus -- each optional, NULL to skip -- valid uint32 [B] = empties mask of the NEW state
 * (valid_actions of the player to move next) and obs_board int8 [B][cells] = the new board with ids relative to the
 * player to move next (state_to_observation, _relative_player_id modulo rel_mod). */
int crl_ttt_step_board(const crl_ctx *ctx, int64_t B, int8_t *board, int8_t *winner, int8_t *to_move, const int8_t *action,
                       int8_t *reward, uint8_t *terminal, int8_t *winners, uint32_t *valid, int8_t *obs_board, int rel_mod,
                       uint32_t flags, void *stream);
/* The single-state form of crl_ttt_step_board, ONE BLOCKING call for a caller whose state lies in crl_host_alloc memory
 * (B = 1; as crl_tron_next_state_inplace64_host: every pointer is such memory with one address for host and GPU): the
 * state -- board, winner, mover, action -- travels BY VALUE in the kernel arguments (no PCIe read before the step) and the
 * kernel publishes completion itself (`seq` into *flag, on which the host spins; timeout_s as crl_stream_wait_mapped).
 * Results as crl_ttt_step_board, visible when the call returns. */
int crl_ttt_step_board_host(const crl_ctx *ctx, int8_t *board, int8_t *winner, int8_t *to_move, const int8_t *action,
                            int8_t *reward, uint8_t *terminal, int8_t *winners, uint32_t *valid, int8_t *obs_board, int rel_mod,
                            uint32_t flags, void *stream, uint32_t *flag, uint32_t seq, double timeout_s);
/* valid_actions (valid uint32 [B] empties mask; may be NULL) and / or state_to_observation (obs_board int8 [B][cells]
 * relative to player[b] modulo rel_mod, absolute ids when player == NULL; may be NULL) of reference-layout boards */
int crl_ttt_observe_board(const crl_ctx *ctx, int64_t B, const int8_t *board, const int8_t *player, int rel_mod,
                          int8_t *obs_board, uint32_t *valid, void *stream);
typedef struct {
    uint32_t *tcount, *tstep, *n_episodes;   /* tcount = the env's rollout step count (RNG counter) */
    uint32_t *win_count;   /* [P][B] */
    uint32_t *draw_count;  /* [B] */
    uint32_t *len_sum;     /* [B] */
    int32_t  *results;     /* [B][3+P] or NULL: packed row n_episodes, len_sum, draw_count, win_count[P] (as crl_tron_stats) */
} crl_ttt_stats;
/* random agent, one Philox call per 8 plies, one 32-bit word per 2: with c = tcount and n = the number of empty cells,
 *   w = Philox(ctr={g, c >> 3, 0, 0x54540000}, seed)[(c >> 1) & 3]
 *   draw = w when c is even, lo32(w * (n + 1)) when c is odd  (what the even ply's extraction hi32(w * (n + 1)) left over,
 *          when that ply was the one before in the same game: the two choices are w's leading digits in the mixed radix
 *          (n + 1, n); the definition does not look back, any ply follows from (seed, g, c, board) alone)
 *   r = mulhi32(draw, n); the ply marks the r-th empty cell in row-major order */
int crl_ttt_rollout(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T,
                    uint32_t *occ, int8_t *winner, int8_t *to_move, crl_ttt_stats stats, void *stream);

/* ------------------------------------------------------------------ one learner against the random agent (turn-based games)
 * crl_ttt_step_single / crl_blokus_step_single: one step of B games in which ONE seat is a learner and every other seat
 * plays the random agent of crl_*_rollout -- the reference's random opponent, random.choice(valid_actions)
 * (examples/blokus_client.py:22-23), under this header's Philox contract.  State layouts are those of the game's other
 * entries; seat int8 [B] is the learner's player id in game b (read modulo P; & 3 for Blokus); tcount uint32 [B] is the
 * step counter of the RNG contract.  With s = seat[b], per game, in one launch:
 *   1. Learner ply: only if learner_action != NULL and to_move[b] == s.  learner_action int64 [B] is applied as the
 *      game's step entry would apply it (the per-game encodings are given below); the ply consumes one value of tcount[b],
 *      exactly as a sampled ply does, so a learner that plays the random agent's own draw reproduces crl_*_rollout.
 *   2. Opponent plies: while to_move[b] != s, the random agent's action at tcount[b] -- what crl_*_sample(advance = 1)
 *      returns on that state -- is applied as crl_*_step applies it.
 *   3. If the game ended in 1. or 2.: done[b] = 1, winners[b] as crl_*_step sets it for the ending ply, reward[b] = the
 *      learner's outcome (below); the game is reset (to_move 0) and 2. goes on until it is the learner's turn.  A fresh game
 *      cannot end within P - 1 plies (TicTacToe: no line in fewer than P + 1 plies as K >= 2, and crl_ttt_step_single
 *      requires cells >= P; Blokus: no player is out of moves in round 0), so one call ends a game at most once.
 *   4. Otherwise reward[b] = 0, done[b] = 0 and winners[b] the step's "no winner" (-1 TicTacToe, 0 Blokus).
 *   5. Always written, of the state the call leaves: the learner's legal moves and its observation (below).
 * learner_action == NULL plays no learner ply: the call that advances a freshly reset batch to the learner's turn.  At most
 * 2 (P - 1) opponent plies are played per call, which no state of the game (to_move in [0, P)) reaches.
 * Argument checks (CRL_EINVAL) before any device work: NULL pointers, unknown flag bits, B out of range, and per game below.
 *
 * TicTacToe: learner_action v in [-1, cells) is played as crl_ttt_step's int8 action v, every other value as -1 (pass:
 * an occupied cell or a pass leaves the board and passes the turn, as there).  reward int8 [B] = +1 if the winner is s,
 * -1 if another player won, 0 for a draw (current_rewards, tictactoe_2p_env.py:233-236); winners int8 [B] as crl_ttt_step.
 * valid uint32 [B] = empties mask; obs_board int8 [B][cells] (4-byte aligned) = crl_ttt_board(player = s, rel_mod).
 * flags must be 0; rel_mod >= 1 (as crl_ttt_step_observe); the context must have cells >= P.  One lane per game; boards of at
 * most 16 cells test for a line with the win-mask table of crl_ttt_create when it lives on the launching device. */
int crl_ttt_step_single(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                        uint32_t *occ, int8_t *winner, int8_t *to_move, const int8_t *seat,
                        const int64_t *learner_action, uint32_t *tcount,
                        int8_t *reward, uint8_t *done, int8_t *winners,
                        int8_t *obs_board, uint32_t *valid, int rel_mod, uint32_t flags, void *stream);

/* ------------------------------------------------------------------ Blokus (20 x 20, 4 players)
 * State (reference BlokusEnvironment.py:283-289: (Board, round_count, [AI x 4])):
 *   occ     uint32 [B][4][20]  bit x of occ[b][c][y] set = cell (x, y) holds colour c+1 (Board.board_contents[y][x])
 *   inv     uint32 [B][4]      bit i set = piece i (inventory order of ai.py:12-22) still held by that player
 *   score   int32  [B][4]      AI.player_score
 *   round   int32  [B]         round_count
 *   to_move int32  [B]
 * Action id = ((piece*400 + y*20 + x)*8 + orientation)*5 + shift for the reference string
 * "{piece};({x}, {y});{orientation}{shift}" (BlokusEnvironment.py:55-80; orientation order board.py:47);
 * ascending ids are exactly the order of BlokusEnvironment.valid_actions; -1 = '' (pass).
 * The step entries also take EXTENDED ids, for indices valid_actions never emits but next_state accepts (it places whatever
 * string_to_action parsed, BlokusEnvironment.py:417-419, and numpy wraps negative indices, board.py:103):
 *   CRL_BLOKUS_EXT_BASE + ((piece*1600 + (y+20)*40 + (x+20))*8 + orientation)*5 + shift,   x, y in [-20, 20).       */
#define CRL_BLOKUS_ACTION_IDS 336000
#define CRL_BLOKUS_MASK_WORDS 10500
#define CRL_BLOKUS_EXT_BASE   336000
#define CRL_BLOKUS_EXT_IDS    1344000                 /* 21 * 1600 * 8 * 5 */
/* per-game codes crl_blokus_step / crl_blokus_step_observe put into reward[b] where the reference's next_state RAISES; the
 * game is left exactly as it was (next_state works on copies, BlokusEnvironment.py:408-409), terminal[b] = winners[b] = 0 */
#define CRL_BLOKUS_INDEX_ERROR -1   /* IndexError: a cell outside numpy's index range [-20, 20) (board.py:103), or a shift id
                                     * that names no cell of the piece (computation.py:218) */
#define CRL_BLOKUS_VALUE_ERROR -2   /* ValueError: piece not in the mover's inventory (ai.py:47 list.remove); the board update
                                     * runs first in the reference, so an IndexError takes precedence */
#define CRL_BLOKUS_BAD_ACTION  -3   /* the id is neither a dense nor an extended id (the reference's KeyError for an unknown
                                     * piece name is the closest relative) */
int crl_blokus_create(crl_ctx **out);
/* The random agent of crl_ttt_rollout as a stand-alone call: action[b] = the r-th empty cell (flat index, row-major
 * np.where order) with r as crl_ttt_rollout's RNG contract defines it for step counter tcount[b], -1 on a full board; advance != 0
 * also increments tcount.  T x (crl_ttt_sample; crl_ttt_step with CRL_STEP_AUTO_RESET) == crl_ttt_rollout(T). */
int crl_ttt_sample(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                   uint32_t *tcount, int advance, int8_t *action, void *stream);

/* DIAGNOSTIC: per-phase shader-cycle sums of crl_blokus_rollout (prep, count, rng, select, apply, exists, rest, -).
 * Returns 1 and the sums only in a library built with -DBLK_STAMPS, else 0 and zeros (the shipped build). */
int crl_blokus_stamps(uint64_t *out8, int reset);
/* HOST helper: cells (dx,dy pairs, 2*n int8) of (piece, orientation, shift) relative to the anchor; returns n.
 * Restates computation.py:184-246 (rotate_default_piece / shift_offsets). */
int crl_blokus_placement(int piece, int orient, int shift, int8_t *cells_xy);
/* replaces BlokusEnvironment.new_state (BlokusEnvironment.py:248-289); mask as for crl_tron_reset */
int crl_blokus_reset(const crl_ctx *ctx, int64_t B, const uint8_t *mask, uint32_t *occ, uint32_t *inv, int32_t *score,
                     int32_t *round, int32_t *to_move, void *stream);
/* replaces BlokusEnvironment.next_state (BlokusEnvironment.py:357-451).  No legality check (the reference
 * leaves that to its caller, match_server.py:193): as there, a placement on occupied cells OVERWRITES them (other colours
 * included) and still scores, cells at x or y in -20..-1 WRAP to the far edge (numpy), and where the reference raises the
 * game stays untouched and reward[b] carries CRL_BLOKUS_INDEX_ERROR / _VALUE_ERROR / _BAD_ACTION (see above).
 * action int32 [B]: dense or extended id, < 0 = '' (pass).  reward int8 [B]: the mover's rank in the ascending score
 * order at terminal, else 0; terminal uint8 [B]: no player has a move on the PRE-move board with the
 * post-move inventories; winners uint8 [B]: bitmask of players whose score equals max(0, best), 0 unless terminal */
int crl_blokus_step(const crl_ctx *ctx, int64_t B, uint32_t *occ, uint32_t *inv, int32_t *score, int32_t *round, int32_t *to_move,
                    const int32_t *action, int8_t *reward, uint8_t *terminal, uint8_t *winners, uint32_t flags, void *stream);
/* replaces BlokusEnvironment.valid_actions / board.get_all_valid_moves (BlokusEnvironment.py:453-500, board.py:170-193)
 * for `player` (int8 [B]; NULL = the player to move): count int32 [B] (may be NULL) and/or the dense id bitmap
 * mask uint32 [B][CRL_BLOKUS_MASK_WORDS] (may be NULL; 42 KB per game, meant for small B). */
int crl_blokus_valid(const crl_ctx *ctx, int64_t B, const uint32_t *occ, const uint32_t *inv, const int32_t *score,
                     const int32_t *round, const int32_t *to_move, const int8_t *player, int32_t *count, uint32_t *mask, void *stream);
/* replaces BlokusEnvironment.state_to_observation (BlokusEnvironment.py:721-768) for observer player[b]:
 * obs_board int8 [B][20][20], 4-byte aligned (-1 empty, else (owner - observer) % 4, rotated by np.rot90(k=-observer)),
 * obs_pieces uint8 [B][4][21] (row r = player (r + observer) % 4), obs_score int32 [B][4] (rolled by -observer) */
int crl_blokus_observe(const crl_ctx *ctx, int64_t B, const uint32_t *occ, const uint32_t *inv, const int32_t *score,
                       const int8_t *player, int8_t *obs_board, uint8_t *obs_pieces, int32_t *obs_score, void *stream);
/* The ordered legal-action LIST, compacted: what BlokusEnvironment.valid_actions returns (BlokusEnvironment.py:453-500,
 * board.py:170-193) in a form a policy can consume for a whole batch.  count int32 [B] = number of legal actions of `player`
 * (int8 [B]; NULL = the player to move); ids int32 [B][cap]: ids[b][0 .. min(count[b], cap)) = their dense ids in
 * ascending order = the reference's order (piece -> anchor row-major -> orientation -> shift); entries beyond are left
 * untouched.  Either output may be NULL; cap in 1..2^28 when ids is given.  (Observed maximum in reference-played games:
 * 1,693 actions; cap = 2048 is safe for play from the empty board; hand-made boards reach 12,952; count tells when a list
 * was cut -- the kernel counts the whole list whatever cap is.) */
int crl_blokus_valid_list(const crl_ctx *ctx, int64_t B, const uint32_t *occ, const uint32_t *inv, const int32_t *score,
                          const int32_t *round, const int32_t *to_move, const int8_t *player, int32_t *ids, int32_t *count,
                          int cap, void *stream);
/* action[b] = dense id of the rank[b]-th (0-based) entry of that list without materialising it, -1 when rank[b] is outside
 * [0, count): "play the r-th legal action" for caller-chosen ranks (crl_blokus_sample draws the rank itself).
 * count (may be NULL) receives the list length. */
int crl_blokus_select(const crl_ctx *ctx, int64_t B, const uint32_t *occ, const uint32_t *inv, const int32_t *score,
                      const int32_t *round, const int32_t *to_move, const int8_t *player, const int32_t *rank,
                      int32_t *action, int32_t *count, void *stream);
/* replaces BlokusEnvironment.is_valid_action (BlokusEnvironment.py:667-719, called per move from match_server.py:193):
 * ok uint8 [B] = 1 iff action[b] (dense id) is in valid_actions(player) -- tested directly (piece held, the shift names a
 * cell of the piece, that cell's target is an anchor, every cell lands on an allowed cell), no enumeration */
int crl_blokus_is_valid(const crl_ctx *ctx, int64_t B, const uint32_t *occ, const uint32_t *inv, const int32_t *score,
                        const int32_t *round, const int32_t *to_move, const int8_t *player, const int32_t *action,
                        uint8_t *ok, void *stream);
/* One step of Board.check_orientation_shifts (board.py:156-168 -> computation.py:144-180 check_shifted): ok uint8 [B] = 1 iff
 * every cell of the placement action[b] names lies on the board, is empty and has no orthogonal neighbour of colour player[b] + 1
 * -- whether or not the index is an anchor and whether or not the piece is held (so: crl_blokus_is_valid minus those two
 * conditions; it needs the row bitboards only). */
int crl_blokus_fits(const crl_ctx *ctx, int64_t B, const uint32_t *occ, const int8_t *player, const int32_t *action, uint8_t *ok,
                    void *stream);
/* occ rows from Board.board_contents as int8 [B][20][20] (0 empty, else colour): the inverse of crl_blokus_board, for
 * callers that hold reference-layout boards */
int crl_blokus_pack(const crl_ctx *ctx, int64_t B, const int8_t *board, uint32_t *occ, void *stream);
/* Board.board_contents as int8 [B][20][20] (0 empty, else colour) */
int crl_blokus_board(const crl_ctx *ctx, int64_t B, const uint32_t *occ, int8_t *board, void *stream);
/* One launch for a ply of every game, as a learner / vector env needs it: [sample ->] next_state -> number of legal actions and
 * state_to_observation of the player to move NEXT.  Exactly equivalent to
 *   [crl_blokus_sample(..., advance = 1);]  crl_blokus_step(..., flags);  crl_blokus_valid(..., player = NULL, count, NULL);
 *   crl_blokus_observe(..., player = to_move, ...)
 * with action == NULL meaning "play the rollout's random agent at tcount[b] and advance tcount" (tcount may be NULL when
 * actions are given).  n_valid int32 [B]; obs_* as crl_blokus_observe (obs_board 4-byte aligned); obs_player int8 [B] = the
 * observer = the player to move. */
int crl_blokus_step_observe(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                            uint32_t *occ, uint32_t *inv, int32_t *score, int32_t *round, int32_t *to_move,
                            const int32_t *action, uint32_t *tcount, int8_t *reward, uint8_t *terminal, uint8_t *winners,
                            int32_t *n_valid, int8_t *obs_board, uint8_t *obs_pieces, int32_t *obs_score, int8_t *obs_player,
                            uint32_t flags, void *stream);
typedef struct {
    uint32_t *tcount, *tstep, *n_episodes;
    uint32_t *win_count;   /* [4][B] */
    uint32_t *len_sum;     /* [B] */
    int32_t  *score_sum;   /* [4][B] final scores summed over finished episodes */
    int32_t  *results;     /* [B][10] or NULL: packed row n_episodes, len_sum, win_count[4], score_sum[4] (as crl_tron_stats) */
} crl_blokus_stats;
/* random agent: the mover plays the r-th action of valid_actions() (reference order), r = mulhi32(w, n), '' if n = 0;
 * w = Philox(ctr={g, c >> 2, 0, 0x424c0000}, seed)[c & 3] with c = tcount; auto-reset on terminal */
int crl_blokus_rollout(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T,
                       uint32_t *occ, uint32_t *inv, int32_t *score, int32_t *round, int32_t *to_move,
                       crl_blokus_stats stats, void *stream);

/* The random agent of crl_blokus_rollout as a stand-alone call: action[b] = dense id of the r-th legal action of the
 * player to move, in reference order, r = mulhi32(Philox(...)[tcount & 3], number of legal actions); -1 (pass, '')
 * when there is none; advance != 0 also increments tcount.
 * T x (crl_blokus_sample; crl_blokus_step with CRL_STEP_AUTO_RESET) == crl_blokus_rollout(T). */
int crl_blokus_sample(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                      const uint32_t *inventory, const int32_t *score, const int32_t *round, const int32_t *to_move,
                      uint32_t *tcount, int advance, int32_t *action, void *stream);

/* crl_blokus_step_single: the contract above for Blokus.  learner_action v: without flags, v in
 * [-1, CRL_BLOKUS_EXT_BASE + CRL_BLOKUS_EXT_IDS) is played as crl_blokus_step's int32 action v, v < -1 is a pass, larger
 * values give CRL_BLOKUS_BAD_ACTION; with CRL_STEP_RANK_ACTION, v is a rank into the learner's ordered legal list (as
 * crl_blokus_select) and a rank outside [0, count) is a pass.  A learner ply that hits a CRL_BLOKUS_*_ERROR code puts it
 * into reward[b]; the state and tcount[b] stay as they were, no opponent plays, done[b] = 0.  At the end of a game reward[b]
 * = the learner's rank in the final scores by crl_blokus_step's rule with the mover replaced by s (what the reference's
 * next_state gives its mover, BlokusEnvironment.py:424-440), whoever made the last ply; winners uint8 [B] as crl_blokus_step.
 * n_valid int32 [B] = the learner's number of legal actions, obs_* = crl_blokus_observe(player = s) (obs_board 4-byte
 * aligned).  One wave per game: the board stays in LDS for every ply of the call (at most 7), and the learner's count and
 * observation are computed from that copy. */
int crl_blokus_step_single(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                           uint32_t *occ, uint32_t *inv, int32_t *score, int32_t *round, int32_t *to_move,
                           const int8_t *seat, const int64_t *learner_action, uint32_t *tcount,
                           int8_t *reward, uint8_t *done, uint8_t *winners, int32_t *n_valid,
                           int8_t *obs_board, uint8_t *obs_pieces, int32_t *obs_score, uint32_t flags, void *stream);

/* ------------------------------------------------------------------ batched random playouts (turn-based games)
 * crl_ttt_playout / crl_blokus_playout: from each of B positions, play R games of the random agent to their end and count
 * who won -- the evaluation step of flat Monte Carlo and of MCTS with random rollouts.  One launch, no host sync.
 *
 * Inputs are read only: the state arrays (occ, winner / inv, score, round, to_move) have the layouts of the game's other
 * entries and are never written.  tcount uint32 [B] is the step-counter base of the RNG contract below; NULL means 0.
 * Rows: cand int32 [B][A], or NULL with A == 1.  Row (b, a) evaluates candidate cand[b][a], a move of the player
 * p0 = to_move[b]; with cand == NULL row (b, 0) evaluates the position as it stands (no candidate ply).
 * Playouts: row (b, a) plays R playouts r = 0 .. R-1, each on a private copy of position b:
 *   1. the candidate ply, if there is a candidate, applied as crl_*_step applies that action; it consumes no random draw;
 *   2. then random-agent plies k = 0, 1, ..., each the random agent's action applied as crl_*_step applies it;
 *   3. the playout stops at the first ply (1. or 2.) that crl_*_step would report terminal; nothing is ever reset.
 * Random stream: ply k of part 2 has step counter c = tcount[b] + k (uint32 arithmetic) and game id g = first_env_id + b
 * (low 32 bits); its draw is the game's random agent (crl_*_rollout, stated with crl_ttt_rollout / crl_blokus_rollout above)
 * with the third counter word (a << 16) | r in place of 0 and its own tag:
 *   TicTacToe  w = Philox(ctr={g, c >> 3, (a << 16) | r, 0x54500000}, seed)[(c >> 1) & 3]; the even / odd mixed-radix rule
 *              and r' = mulhi32(draw, n) are crl_ttt_rollout's: the ply marks empty cell number r' in row-major order;
 *   Blokus     w = Philox(ctr={g, c >> 2, (a << 16) | r, 0x42500000}, seed)[c & 3]; the mover plays legal action number
 *              mulhi32(w, n) of its n legal actions in reference order, '' (pass) when n = 0, as crl_blokus_rollout.
 * So with cand == NULL a playout is crl_*_rollout on a copy of the state under that counter and tag, stopped at its first
 * terminal ply.
 * Outputs, every row written (overwritten, never accumulated; a skipped row holds zeros):
 *   played  uint32 [B][A]     R, or 0 when the row is skipped;
 *   wins    uint32 [B][A][P]  playouts won by player p: TicTacToe the terminal step's winner (draws are
 *                             played - sum_p wins); Blokus bit p of the terminal step's winners mask, so a tie counts for
 *                             every tied player;
 *   len_sum uint32 [B][A]     plies played over the R playouts, the candidate ply included;
 *   score_sum int32 [B][A][4] (Blokus) the sum of the final score[c].
 * Argument checks (CRL_EINVAL, with a crl_last_error message, before any device work): NULL state / output pointers, B out
 * of range (as the game's other entries), R or A outside [1, 65535], A != 1 with cand == NULL, flags != 0, and per game below.
 * Lanes are indexed with 64-bit arithmetic: B * A * R may pass 2^31.
 *
 * TicTacToe: a candidate is played only if it lies in [0, cells) and names an empty cell; any other value (-1 padding
 * included) skips its row.  A position that is over (winner[b] >= 0, or no empty cell) or whose to_move[b] is outside
 * [0, P) skips every row.  The context must have cells >= P (as crl_ttt_step_single).  One lane per playout, flat lane
 * index (b, a, r) with r fastest; boards of at most 16 cells test for a line with the win-mask table of crl_ttt_create when
 * it lives on the launching device.  A wave's outcomes are summed per row inside the wave (ballots) before one store or
 * integer atomic per row segment and output word, so the results do not depend on the order of the waves. */
int crl_ttt_playout(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                    const uint32_t *occ, const int8_t *winner, const int8_t *to_move, const uint32_t *tcount,
                    const int32_t *cand, int A, int R,
                    uint32_t *wins, uint32_t *played, uint32_t *len_sum, uint32_t flags, void *stream);
/* Blokus: the mover is p0 = to_move[b] & 3.  A candidate is played only if it is a dense id (< CRL_BLOKUS_EXT_BASE) that
 * is a legal action of p0 by crl_blokus_is_valid's definition; anything else skips its row.  Blokus keeps no "game over"
 * field, so a finished position needs no special case: its first random ply is a pass and the step reports it terminal.
 * One wave per playout with the board in LDS; each ply is crl_blokus_rollout's. */
int crl_blokus_playout(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                       const uint32_t *occ, const uint32_t *inv, const int32_t *score, const int32_t *round,
                       const int32_t *to_move, const uint32_t *tcount,
                       const int32_t *cand, int A, int R,
                       uint32_t *wins, uint32_t *played, uint32_t *len_sum, int32_t *score_sum,
                       uint32_t flags, void *stream);

/* ------------------------------------------------------------------ the tactical (win-or-block) agent of TicTacToe
 * The standard scripted opponent of k-in-a-row games: take a winning cell if there is one, else block the next player who
 * has one, else play at random.  No reference counterpart (the reference's only TicTacToe opponent is the random agent).
 * Per game b with n cells and P players: o[q] = player q's marks, all = OR_q o[q], E = full & ~all (the empty cells), and
 * win(m) = "m holds a K-window that stays on the board", exactly the test crl_ttt_step applies.
 * Winning cells:  W_q = { e in E : win(o[q] | 1 << e) }, as a mask.
 * Tactical move of the mover p = to_move[b] at step counter c of global game g = first_env_id + b:
 *   1. p outside [0, P) or E == 0: the action is -1 (pass) and no draw is made.
 *   2. w = Philox4x32-10(ctr = {g, c >> 1, c2, TAG}, key = {seed lo, seed hi}); u = w[2 (c & 1)], v = w[2 (c & 1) + 1]: one
 *      Philox block per two plies.  crl_ttt_sample_tactical / _rollout_tactical / _step_single_tactical: c2 = 0 and
 *      TAG = 0x54630000; crl_ttt_playout_tactical: c2 = (a << 16) | r and TAG = 0x54430000.  (The random agent's contract
 *      above is untouched.)
 *   3. noisy  iff  u < thr,  thr = min(2^32, ceil(noise * 2^32)) computed on the host in 64 bits, as crl_tron_sample_avoid:
 *      noise = 0 is never noisy, noise = 1 always.
 *   4. noisy: S = E.  Else S = the first non-empty set of W_p, W_{(p+1) mod P}, ..., W_{(p+P-1) mod P} -- the mover's own win
 *      first, then the threat of the earliest player to come -- and S = E when all are empty.
 *   5. the action is the mulhi32(v, popcount(S))-th set bit of S, ascending (row-major order).
 * The agent reads occ and to_move only; like crl_ttt_sample it does not look at winner.
 * Errors (CRL_EINVAL, with a crl_last_error message, before any device work): NULL pointers, B out of range, noise outside
 * [0, 1] or NaN, and what the random-agent sibling of each entry checks (flags != 0, T, A, R, rel_mod, cells >= P).
 * One lane per game (the playout: per playout).  W_q is computed with shift-ANDs per line direction on every board; the
 * entries that play plies test a ply's win as their random siblings do (boards of at most 16 cells: the win-mask table of
 * crl_ttt_create when it lives on the launching device).
 *
 * crl_ttt_winning_cells: cells uint32 [P][B] = W_q of every player, for observations and action priors. */
int crl_ttt_winning_cells(const crl_ctx *ctx, int64_t B, const uint32_t *occ, uint32_t *cells, void *stream);
/* action[b] = the tactical move at step counter tcount[b]; advance != 0 also increments tcount (passes included), as
 * crl_ttt_sample does. */
int crl_ttt_sample_tactical(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                            const int8_t *to_move, uint32_t *tcount, int advance, double noise, int8_t *action, void *stream);
/* crl_ttt_rollout with EVERY seat on the tactical agent: the same auto-reset, crl_ttt_stats bookkeeping and results row,
 * tcount advances by one per ply.
 * T x (crl_ttt_sample_tactical(advance = 1); crl_ttt_step with CRL_STEP_AUTO_RESET) == crl_ttt_rollout_tactical(T). */
int crl_ttt_rollout_tactical(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T, double noise,
                             uint32_t *occ, int8_t *winner, int8_t *to_move, crl_ttt_stats stats, void *stream);
/* crl_ttt_step_single word for word, except that in its step 2 the opponents' action is what
 * crl_ttt_sample_tactical(advance = 1) returns on that state.  The learner's ply still consumes one counter value. */
int crl_ttt_step_single_tactical(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                                 uint32_t *occ, int8_t *winner, int8_t *to_move, const int8_t *seat,
                                 const int64_t *learner_action, uint32_t *tcount,
                                 int8_t *reward, uint8_t *done, int8_t *winners,
                                 int8_t *obs_board, uint32_t *valid, int rel_mod, double noise, uint32_t flags, void *stream);
/* crl_ttt_playout word for word (rows, skipping, outputs, wave-order independence, 64-bit lane indexing), except that every
 * ply after the candidate is the tactical move at step counter c = tcount[b] + k under the playout tag (2. above). */
int crl_ttt_playout_tactical(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                             const uint32_t *occ, const int8_t *winner, const int8_t *to_move, const uint32_t *tcount,
                             const int32_t *cand, int A, int R,
                             uint32_t *wins, uint32_t *played, uint32_t *len_sum, double noise, uint32_t flags, void *stream);

/* ------------------------------------------------------------------ batched Monte Carlo tree search (UCT), TicTacToe
 * crl_ttt_mcts: from each of B positions build a search tree of its own by S simulations s = 0 .. S-1, in order, each
 * evaluated by R random playouts, and report the root's children.  One launch, no host sync.  Added under revision 113: new
 * entries and one new Philox tag, no existing struct, argument list or RNG contract changed.
 * The state is read only, in the layouts of crl_ttt_playout; tcount uint32 [B] may be NULL, which means 0.
 *
 * Nodes.  Node 0 is the root, position b.  A node holds n, the number of simulations that passed through it; w, the
 * half-points of the player who made the move INTO it (a won playout counts 2, a drawn one 1; the root's w stays 0); and
 * one child slot per cell, empty ("none") at first.
 * Descent.  A simulation starts at the root with a private copy of the position.  At node v with the empty cells E of the
 * position there, in ascending order:
 *   expand: if some cell of E has no child, take the lowest such cell e; a new node with the next free index becomes v's
 *           child at e, ply e is played as crl_ttt_step plays it, and the new node is the leaf (also when that ply is
 *           terminal);
 *   select: else take the child u at the cell of E that maximises score(v, u), ties to the lowest cell, and play that cell;
 *           if crl_ttt_step reports the ply terminal u is the leaf, else the descent continues at u.
 * Score, in 64-bit integers with floor divisions:
 *   exploit = (w_u << 15) / (n_u * R)                                        in [0, 65536]
 *   lg(n), n >= 1: m = the index of n's leading one, f = ((n << (31 - m)) >> 23) & 255 (the 8 bits below it, zero-filled),
 *           lg(n) = 256 m + f: a piecewise-linear log2 with 8 fraction bits
 *   X = (lg(n_v) << 24) / n_u
 *   score = exploit + ((cexp * isqrt(X)) >> 8),  isqrt the exact floor square root
 * so cexp / 256 multiplies sqrt(log2 n_v / n_u) on a value scale of 0 .. 1: cexp = 256 is the usual choice, 0 pure
 * exploitation.
 * Evaluation of the leaf L at depth d (plies from the root).  If the ply into L ended the game, all R playouts have that
 * outcome and no draw is made.  Else R playouts r = 0 .. R-1 start from L's position, each the random agent of
 * crl_ttt_rollout played to the first terminal ply: random ply k has step counter c = tcount[b] + d + k (uint32 arithmetic),
 * game id g = first_env_id + b (low 32 bits) and
 *   w = Philox4x32-10(ctr = {g, c >> 3, (s << 16) | r, 0x544D0000}, key = {seed lo, seed hi})[(c >> 1) & 3],
 * with the rollout's even / odd mixed-radix rule and r' = mulhi32(draw, n_empty).  The tag 0x544D0000 is used nowhere else.
 * Backup.  Every node on the path from the root to L: n += 1; every one but the root, q the player who moved into it:
 * w += 2 * (playouts q won) + (playouts drawn).
 * Outputs, every word overwritten:
 *   visits uint32 [B][cells], value uint32 [B][cells]   n and w of the root's child at each cell, 0 where there is none;
 *   nodes  uint32 [B]                                   the node count, root included;
 *   best   int32  [B]                                   the cell whose root child has the most visits; ties go to the larger
 *                                                       w, then to the lowest cell.
 * A position that is over (winner[b] >= 0, or no empty cell) or whose to_move[b] is outside [0, P) is skipped: zeros,
 * nodes 0, best -1.
 * Limits (CRL_EINVAL, with a crl_last_error message, before any device work): NULL state or output pointers, B out of range
 * (as the siblings), S outside [1, S_max], R outside [1, 1024], cexp > 65535, flags != 0, a context with cells < P (as
 * crl_ttt_playout).  S_max = min(4095, 65536 / (8 + 2 * cells) - 1): a tree of S + 1 nodes of 8 + 2 * cells bytes fits one
 * workgroup's 64 KB of LDS, and s fits its counter word -- 2,519 on 3x3, 1,723 on 3x5, 1,128 on 5x5, 1,056 on 3x3x3, 909 on
 * 32 cells.  crl_ttt_mcts_max_simulations returns S_max of the context (a negative code on a bad context).
 * One wave per tree, the tree in LDS: the wave's lanes are the cells while it selects (the arg-max is a cross-lane
 * reduction, the tie rule part of the reduced key), the playouts while it evaluates (R > 64 in passes) and the path
 * entries while it backs up.  Nothing is shared between waves, so the results do not depend on their order. */
int crl_ttt_mcts_max_simulations(const crl_ctx *ctx);
int crl_ttt_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                 const uint32_t *occ, const int8_t *winner, const int8_t *to_move, const uint32_t *tcount,
                 int S, int R, uint32_t cexp,
                 uint32_t *visits, uint32_t *value, uint32_t *nodes, int32_t *best,
                 uint32_t flags, void *stream);

/* ------------------------------------------------------------------ tree search valued by the caller's network (PUCT), TicTacToe
 * crl_ttt_puct_*: B search trees that stay in device memory between launches.  One launch (select) descends every tree to a
 * leaf and writes the leaves out in observation layout; the caller runs its network on that batch, on the same stream; a
 * second launch (backup) expands the leaves with the returned priors and backs the returned values up.  Two launches per
 * simulation for the whole batch, no host synchronisation, capturable into a graph.  The search draws nothing: its contract
 * is integer arithmetic alone.  Added under revision 113: five new entries, no new Philox tag, no existing struct, argument
 * list or RNG contract changed.
 * `tree` is a caller-owned device buffer of B * crl_ttt_puct_tree_bytes(ctx, S_cap) bytes, 16-byte aligned.  Its layout is
 * the library's own business and is opaque to the caller (DESIGN.md 4.5j states it).  Every call on a buffer takes the
 * S_cap, the B and the context that crl_ttt_puct_begin took.
 *
 * Tree and nodes
 * - `begin` copies position b into tree b: the P occupancy words and the mover. No later call reads the game state, so the
 *   batch may be stepped while a search is open.
 * - `begin` makes node 0 the root. The root is *unexpanded*, with n = 0, node count 1 and simulation count 0.
 * - A position that is over (`winner[b] >= 0`, or no empty cell), or whose `to_move[b]` is outside [0, P), makes a *skipped*
 *   tree. Its node count is 0, every later call leaves it alone, and `root` reports zeros and `best` -1.
 * - A node holds n (uint32), w (uint32), one prior slot (uint16) per cell and one child slot (uint16, 0 = none) per cell. w is
 *   the summed value of the player who moved INTO it, on the 0..65536 scale.
 * - A node is *expanded* once a backup has given it priors.
 *
 * `select`, simulation s
 * - The descent starts at the root on a private copy of the root position.
 * - At node v:
 *   - If v is unexpanded, v is the leaf and it is *pending*.
 *   - Otherwise score every empty cell e of the position at v. Take the greatest score, ties to the lowest cell.
 *   - If v has no child at e, a new unexpanded node with the next free index becomes that child.
 *   - Play e as `crl_ttt_step` plays it.
 *   - If that ply ends the game, the child is the leaf, it is *terminal* and not pending. Otherwise the descent continues
 *     at the child.
 * - The score is in 64-bit integers with floor divisions. Let n_u, w_u be those of the child at e, or 0, 0 where there is
 *   none. Let P_e be v's stored prior at e.
 *   - `exploit = n_u ? w_u / n_u : fpu`
 *   - `explore = (cpuct * P_e * isqrt(n_v << 16)) / ((1 + n_u) << 16)`, with isqrt the exact floor root
 *   - `score = exploit + explore`
 *   - `cpuct = 256` is c = 1.0.
 * - The path (at most cells + 1 node indices) and the leaf's kind are kept in the tree until `backup`.
 * - A `select` on a tree with a path outstanding drops that path and descends again. Nothing has changed, so it arrives at
 *   the same leaf.
 * - A tree whose simulation count has reached `S_cap` is not descended: no path, pending 0.
 * - Outputs, every word overwritten. For a pending leaf with mover m:
 *   - `board` int8 [B][cells], relative to m under `rel_mod`, exactly as `crl_ttt_board` writes it.
 *   - `valid` uint32 [B], the empties mask.
 *   - `mover` int8 [B] = m.
 *   - `pending` uint8 [B] = 1.
 *   - `leaf_occ` uint32 [P][B], the leaf position in the state layout, so that it can be handed to any other entry.
 *   - For every other tree: zeros, `mover` -1, `pending` 0.
 *
 * `backup`
 * - A tree without an outstanding path is left alone.
 * - Pending leaf L with empties E and mover m:
 *   - Let SUM = sum over e in E of `prior[b][e]`, with `prior` uint16 [B][cells]; entries at occupied cells are ignored.
 *   - For e in E, L's prior slot is `min(65535, (prior[e] << 16) / SUM)`, or `min(65535, 65536 / |E|)` when SUM = 0. Other
 *     slots are 0.
 *   - L becomes expanded.
 *   - The value of player (m + j) mod P is `value[b][j]` clamped to [0, 65536], with `value` int32 [B][P].
 * - Terminal leaf:
 *   - `prior` and `value` are not read.
 *   - The winner's value is 65536 and every other player's is 0.
 *   - A draw gives every player 32768.
 * - Every node on the path gets n += 1.
 * - Every node on the path but the root gets w += the value of the player who moved into it.
 * - The simulation count goes up by 1 and the path is cleared.
 *
 * `root`, every word overwritten
 * - `visits`, `value` uint32 [B][cells]: n and w of the root's child at each cell, 0 where there is none.
 * - `prior` uint32 [B][cells]: the root's stored priors.
 * - `nodes`, `sims` uint32 [B].
 * - `best` int32 [B]: the cell of the most visited child, ties to the larger w, then to the lowest cell. -1 when no child has
 *   a visit.
 *
 * Refused with `CRL_EINVAL` and a `crl_last_error` message, before any device work
 * - NULL pointers, other than `leaf_occ`.
 * - A `tree` pointer that is not 16-byte aligned.
 * - B out of range, as the siblings define it.
 * - `S_cap` outside [1, 4095]. Child slots are 16 bits and w stays below 2^32. A wider index is a later change.
 * - `cpuct` > 65535.
 * - `fpu` > 65536.
 * - `rel_mod` as `crl_ttt_board` checks it (>= 1: the board is always relative to a player here).
 * - `flags != 0`.
 * - A context with cells < P, or a context that is not tictactoe.
 * crl_ttt_puct_tree_bytes returns the bytes of ONE tree, a multiple of 16 that grows with S_cap, or a negative code (a bad
 * context, S_cap out of range).
 * One wave per tree in every kernel, 64-bit tree offsets, grid-stride loops; nothing is shared between waves, so the results
 * do not depend on their order. */
int64_t crl_ttt_puct_tree_bytes(const crl_ctx *ctx, int S_cap);
int crl_ttt_puct_begin(const crl_ctx *ctx, int64_t B, const uint32_t *occ, const int8_t *winner, const int8_t *to_move,
                       int S_cap, void *tree, void *stream);
int crl_ttt_puct_select(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, uint32_t cpuct, uint32_t fpu, int rel_mod,
                        int8_t *board, uint32_t *valid, int8_t *mover, uint8_t *pending, uint32_t *leaf_occ /* may be NULL */,
                        uint32_t flags, void *stream);
int crl_ttt_puct_backup(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, const uint16_t *prior, const int32_t *value,
                        uint32_t flags, void *stream);
int crl_ttt_puct_root(const crl_ctx *ctx, int64_t B, void *tree, int S_cap,
                      uint32_t *visits, uint32_t *value, uint32_t *prior, uint32_t *nodes, uint32_t *sims, int32_t *best,
                      void *stream);

/* ------------------------------------------------------------------ tree search valued by the caller's network (PUCT), Tron
 * crl_tron_puct_*: crl_ttt_puct_*'s design for ONE seat of Tron.  B search trees stay in device memory between launches; one
 * launch (select) descends every tree to a leaf and writes the leaves out in observation layout; the caller runs its network
 * on that batch, on the same stream; a second launch (backup) expands the leaves with the returned priors and backs the
 * returned values up.  Two launches per simulation for the whole batch, no host synchronisation, capturable into a graph.
 * Added under revision 113: five new entries, no new Philox tag, no existing struct, argument list or RNG contract changed.
 * As in crl_tron_mcts the tree branches on the seat's three actions only.  Every other player is part of the transition,
 * played by a scripted MODEL (the random or the avoid agent) from counter-based draws, so a node's position is a pure function
 * of the root and the edge sequence: a tree holds the root position and no other, and `select` replays the edges.
 * `tree` is a caller-owned device buffer of B * crl_tron_puct_tree_bytes(ctx, S_cap) bytes, 16-byte aligned.  Its layout is
 * the library's own business and is opaque to the caller (DESIGN.md 4.5k states it).  Every call on a buffer takes the
 * S_cap, the B and the context that crl_tron_puct_begin took.
 *
 * Tree and nodes
 * - `begin` copies into tree b everything a later call needs: the root board bytes, heads (clamped onto the board,
 *   crl_tron_playout's precondition), dirs & 3, deaths, `tcount[b]` (NULL means 0), the seat `seat[b]` (NULL means player 0),
 *   g = the low 32 bits of `first_env_id + b`, the seed, the model (with CRL_PLAYOUT_AVOID the avoid agent with `noise`, else
 *   the random agent; noise is checked and otherwise unused) and the noise threshold.  The state has crl_tron_step's layouts
 *   and is read only.  No later call reads the game state, so the batch may be stepped while a search is open.
 * - `begin` makes node 0 the root. The root is *unexpanded*, with n = 0, node count 1 and simulation count 0.
 * - A position is skipped when the seat is outside [0, P), the seat is dead (deaths[seat][b] != 0), or P >= 2 and fewer than
 *   two players are alive (crl_tron_mcts's rule).  It makes a *skipped* tree. Its node count is 0, every later call leaves it
 *   alone, and `root` reports zeros and `best` -1.
 * - A node holds n (uint32), w (uint32), three prior slots (uint16) and three child slots (uint16, 0 = none), for the actions
 *   0 forward, 1 right, 2 left (crl_tron_step_single's encoding). w is the seat's summed value on the 0..65536 scale.
 * - A node is *expanded* once a backup has given it priors.
 *
 * `select`, simulation s
 * - The descent starts at the root on a private copy of the root position.
 * - At node v at depth k (edges from the root):
 *   - If v is unexpanded, v is the leaf and it is *pending*.
 *   - Otherwise score the three actions e. Take the greatest score, ties to the lowest action.
 *   - If v has no child at e, a new unexpanded node with the next free index becomes that child.
 *   - Play the tree step e, which is crl_tron_mcts's tree step: its step counter is c = tcount + k (uint32 arithmetic).  The
 *     seat plays e.  Every other live player q plays the model agent, decided on the pre-step position:
 *       random  W = Philox4x32-10(ctr = {g, c >> 3, 0xFFFF0000, 0x54700000 | (q >> 2)}, key = {seed lo, seed hi}), then
 *               crl_tron_rollout's digit rule with j = c & 7 and q & 3;
 *       avoid   W = Philox4x32-10(ctr = {g, c, 0xFFFF0000, 0x54610000 | q}, key = {seed lo, seed hi}), then
 *               crl_tron_sample_avoid's rule (threshold, clamped probes, side bit).
 *     The step itself is crl_tron_step without reset, with owners: the board keeps the player ids and the killer ids in
 *     `deaths` come out exactly as crl_tron_step writes them.
 *   - If the node reached is CLOSED (the seat is dead or at most one player is alive), the child is the leaf, it is *terminal*
 *     and not pending, and its value is 65536 iff the seat is alive, else 0. Otherwise the descent continues at the child.
 * - The score is in 64-bit integers with floor divisions. Let n_u, w_u be those of the child at e, or 0, 0 where there is
 *   none. Let P_e be v's stored prior at e.
 *   - `exploit = n_u ? w_u / n_u : fpu`
 *   - `explore = (cpuct * P_e * isqrt(n_v << 16)) / ((1 + n_u) << 16)`, with isqrt the exact floor root
 *   - `score = exploit + explore`
 *   - `cpuct = 256` is c = 1.0.
 * - The path (at most S_cap + 1 node indices) and the leaf's kind are kept in the tree until `backup`.
 * - A `select` on a tree with a path outstanding drops that path and descends again. Nothing has changed, so it arrives at
 *   the same leaf.
 * - A tree whose simulation count has reached `S_cap` is not descended: no path, pending 0.
 * - Outputs, every word overwritten. For a pending leaf:
 *   - `obs_board` int8 [B][N*N], `obs_heads` int16 [P][B], `obs_dirs` int8 [P][B], `obs_deaths` int8 [P][B]: exactly what
 *     crl_tron_observe with `player[b]` = the seat writes for the leaf position.
 *   - `pending` uint8 [B] = 1.
 *   - `depth` uint32 [B]: the edges from the root to the leaf, so the leaf's counter base is `tcount + depth`.
 *   - `leaf_board`, `leaf_heads`, `leaf_dirs`, `leaf_deaths` (all four NULL, or none): the leaf position in the state layout,
 *     so that it can be handed to crl_tron_territory, crl_tron_playout or any other entry.
 *   - For every other tree: zeros, `pending` 0.
 *
 * `backup`
 * - A tree without an outstanding path is left alone.
 * - Pending leaf L:
 *   - Let SUM = `prior[b][0] + prior[b][1] + prior[b][2]`, with `prior` uint16 [B][3].
 *   - L's prior slot at a is `min(65535, (prior[b][a] << 16) / SUM)`, or `min(65535, 65536 / 3)` each when SUM = 0.
 *   - L becomes expanded.
 *   - The value is `value[b]` clamped to [0, 65536], with `value` int32 [B]: the seat's.
 * - Terminal leaf: `prior` and `value` are not read. The value is 65536 iff the seat is alive, else 0.
 * - Every node on the path gets n += 1.
 * - Every node on the path but the root gets w += the value.
 * - The simulation count goes up by 1 and the path is cleared.
 *
 * `root`, every word overwritten
 * - `visits`, `value` uint32 [B][3]: n and w of the root's child at each action, 0 where there is none.
 * - `prior` uint32 [B][3]: the root's stored priors.
 * - `nodes`, `sims` uint32 [B].
 * - `best` int32 [B]: the most visited action, ties to the larger w, then to the lower action. -1 when no child has a visit.
 *
 * Refused with `CRL_EINVAL` and a `crl_last_error` message, before any device work
 * - NULL pointers, other than `tcount`, `seat` and the leaf_* set.
 * - A leaf_* set that is partly NULL.
 * - A `tree` pointer that is not 16-byte aligned.
 * - B out of range, as the siblings define it.
 * - `S_cap` outside [1, 4095]. Child slots are 16 bits and w stays below 2^32. A wider index is a later change.
 * - `cpuct` > 65535.
 * - `fpu` > 65536.
 * - `noise` outside [0, 1] or NaN.
 * - Flags other than CRL_PLAYOUT_AVOID in `begin`; `flags != 0` elsewhere.
 * - A context that is not a Tron context.
 * A board whose byte copy (N*N rounded up to 16, plus 16 bytes) does not fit the 64 KB of one workgroup's LDS answers
 * CRL_EUNSUPPORTED: that is N >= 256, beyond the N <= 181 of crl_tron_create, so every Tron context is supported.
 * A board value outside 0..P is wrong input: the results are unspecified, and it is never a wild access.
 * crl_tron_puct_tree_bytes returns the bytes of ONE tree, a multiple of 16 that grows with S_cap, or a negative code (a bad
 * context, S_cap out of range).
 * One wave per tree in every kernel, one to four waves per workgroup (as many byte boards as fit), 64-bit tree offsets,
 * grid-stride loops; nothing is shared between waves, so the results do not depend on their order. */
int64_t crl_tron_puct_tree_bytes(const crl_ctx *ctx, int S_cap);
int crl_tron_puct_begin(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                        const int8_t *board, const int16_t *heads, const int8_t *dirs, const int8_t *deaths,
                        const uint32_t *tcount /* may be NULL */, const int8_t *seat /* may be NULL */,
                        int S_cap, double noise, uint32_t flags, void *tree, void *stream);
int crl_tron_puct_select(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, uint32_t cpuct, uint32_t fpu,
                         int8_t *obs_board, int16_t *obs_heads, int8_t *obs_dirs, int8_t *obs_deaths,
                         uint8_t *pending, uint32_t *depth,
                         int8_t *leaf_board, int16_t *leaf_heads, int8_t *leaf_dirs, int8_t *leaf_deaths /* all four NULL, or none */,
                         uint32_t flags, void *stream);
int crl_tron_puct_backup(const crl_ctx *ctx, int64_t B, void *tree, int S_cap, const uint16_t *prior, const int32_t *value,
                         uint32_t flags, void *stream);
int crl_tron_puct_root(const crl_ctx *ctx, int64_t B, void *tree, int S_cap,
                       uint32_t *visits, uint32_t *value, uint32_t *prior, uint32_t *nodes, uint32_t *sims, int32_t *best,
                       void *stream);

/* ------------------------------------------------------------------ batched tree search with progressive widening, Blokus
 * crl_blokus_mcts: from each of B positions build a search tree of its own by S simulations s = 0 .. S-1, in order, each
 * evaluated by R random playouts, and report the root's children.  One launch, no host sync, capturable into a graph.  Added
 * under revision 113: new entries only, no new Philox tag, no existing struct, argument list or RNG contract changed.
 * The state is read only, in the layouts of crl_blokus_playout; tcount uint32 [B] may be NULL, which means 0.
 *
 * Nodes.  Node 0 is the root, position b.  A node holds n, the number of simulations that passed through it; w, the playouts
 * won by the player who made the move INTO it (bit q of the terminal winners mask, so a tie counts for every tied player;
 * the root's w stays 0); and an ordered list of children, empty at first.  For a node v: p_v is its mover, L_v the number
 * of legal actions of p_v there (crl_blokus_valid's count), d_v its depth in plies from the root.
 * Children.  A position has hundreds of legal actions, so a node is widened progressively: it gets its k-th child only
 * once it has been visited about k^2 times, and that child is a uniformly drawn legal action.
 *   widening node (every node; the root when cand == NULL): cap = min(W, max(L_v, 1)).  With c children and n visits so far
 *     (this simulation not counted) the node EXPANDS iff c < cap and c * c <= n, else it SELECTS.  The new child is the pass
 *     (id -1) when L_v == 0; else u = Philox4x32-10(ctr = {g, 0x80000000 | d_v, s, 0x42500000}, key = {seed lo, seed hi})[0],
 *     rho = mulhi32(u, L_v), and while rho is the rank of an existing child of v: rho = (rho + 1) mod L_v; the child is legal
 *     action number rho of p_v in reference order (crl_blokus_select's answer), appended as slot c.
 *   candidate root (cand != NULL, int32 [B][A], 1 <= A <= 64): column a is PLAYABLE iff cand[b][a] is a legal dense id of the
 *     mover (crl_blokus_is_valid) and differs from every earlier playable column of the row.  The root expands the lowest
 *     playable column that has no child; when all have one it selects.  Slot = column.  The nodes below the root widen as
 *     above.  A row with no playable column is skipped: every slot empty, nodes 0, best -2.
 * Descent.  A simulation starts at the root on a private copy of the position.
 *   expand: the new child's ply is played as crl_blokus_step plays it; the child is the leaf, also when that ply is terminal.
 *   select: the child with the greatest score(v, u) is taken, ties to the lowest slot, and its ply is played; if the ply is
 *           terminal that child is the leaf, else the descent continues there.
 * Score, crl_ttt_mcts's with wins counting 1, in 64-bit integers with floor divisions (lg and isqrt as stated there):
 *   exploit = (w_u << 16) / (n_u * R),  X = (lg(n_v) << 24) / n_u,  score = exploit + ((cexp * isqrt(X)) >> 8).
 * Evaluation of the leaf at depth d.  A terminal ply gives all R playouts its winners mask, and nothing is drawn.  Else R
 * playouts r = 0 .. R-1, each crl_blokus_playout's random ply loop from the leaf's position to the first terminal ply:
 * ply k has step counter c = tcount[b] + d + k (uint32 arithmetic), game id g = first_env_id + b (low 32 bits) and
 *   w = Philox4x32-10(ctr = {g, (c >> 2) | 0x40000000, (s << 16) | r, 0x42500000}, key = {seed lo, seed hi})[c & 3];
 * the mover plays legal action number mulhi32(w, n) of its n legal actions in reference order, '' (pass) when n = 0.
 * Counter space: crl_blokus_playout's second counter word is c >> 2 < 2^30; the search sets bit 30 (playouts) or bit 31
 * (widening draws) of that word, so under the shared tag 0x42500000 no block of one is a block of the other.
 * Backup.  Every node on the path: n += 1; every one but the root, q the player who moved into it: w += the playouts whose
 * winners mask has bit q.
 * Outputs, every word overwritten; K = A with candidates, else W:
 *   ids    int32  [B][K]   the child's dense id, -1 for the pass, -2 for an empty slot;
 *   visits uint32 [B][K], value uint32 [B][K]   the child's n and w, 0 for an empty slot;
 *   nodes  uint32 [B]      the node count, root included;
 *   best   int32  [B]      the id of the root child with the most visits; ties go to the larger w, then to the lowest slot.
 * Blokus keeps no "game over" field, so a finished position is not special: its root gets the pass as its only child and
 * that ply is terminal.
 * Limits (CRL_EINVAL, with a crl_last_error message, before any device work): NULL state or output pointers, B out of range
 * (as the siblings), A outside [1, 64] with cand or A != 1 without it, W outside [1, 64], S outside [1, S_max], R outside
 * [1, 1024], cexp > 65535, flags != 0, a context that is not a Blokus one.
 * S_max = min(65535, (45056 - 1280) / 24 - 1) = 1823: a node takes 24 bytes of LDS (n, w, id, rank, L_v, and parent / slot /
 * terminal / child count in one word), a tree besides its S + 1 nodes 1,280 bytes (the path of at most min(S, 336) plies --
 * 84 placements exist and at most three passes separate two of them --, the playout counts, the child slots of the node
 * being looked at), and the trees of a workgroup get 45,056 bytes of its 64 KB beside the piece tables and the four waves'
 * boards; s has 16 bits in its counter word.  crl_blokus_mcts_max_simulations returns S_max (a negative code on a bad
 * context).
 * The tree lives in LDS.  R < 4: one wave per tree, as many trees per workgroup (up to four) as fit; R >= 4: one workgroup
 * per tree, every wave replaying the descent on its own board and taking every fourth playout, wave 0 writing the tree
 * between workgroup barriers.  Both give the same bits.  The wave's lanes are the children while it selects (the arg-max is
 * a cross-lane reduction, ties by the lowest lane) and while it probes the ranks.  A node caches its id, its rank, L_v once
 * counted and whether the ply into it was terminal, so a descent through existing nodes only places pieces.  Nothing is
 * shared between trees, so the results do not depend on the order of the waves. */
int crl_blokus_mcts_max_simulations(const crl_ctx *ctx);
int crl_blokus_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                    const uint32_t *occ, const uint32_t *inv, const int32_t *score, const int32_t *round,
                    const int32_t *to_move, const uint32_t *tcount,
                    const int32_t *cand, int A, int W, int S, int R, uint32_t cexp,
                    int32_t *ids, uint32_t *visits, uint32_t *value, uint32_t *nodes, int32_t *best,
                    uint32_t flags, void *stream);

/* ------------------------------------------------------------------ the tree search as a seated agent of Blokus
 * The search of crl_blokus_mcts in the three forms the random agent has: one step, a fused rollout with every seat on it, and
 * the opponents of the single-player step.  Added under revision 113: new entries only, no new Philox tag, no existing
 * struct, argument list or RNG contract changed.
 * The search agent has the parameters W, S, R, cexp (crl_blokus_mcts's) and noise in [0, 1].  Its move for the mover
 * p = to_move[b] & 3 at step counter c of global game g = first_env_id + b (low 32 bits):
 *   1. n = the number of legal actions of p (crl_blokus_valid's count).  n == 0: the action is -1 (the pass); nothing is
 *      drawn and nothing is searched.  (crl_blokus_mcts would answer the same: the pass would be the root's only child.)
 *   2. u = Philox4x32-10(ctr = {g, 0xC0000000 | (c >> 2), 0, 0x42500000}, key = {seed lo, seed hi})[c & 3].  Both top bits
 *      of the second counter word are set: crl_blokus_playout has neither, the search's playouts set only bit 30 and its
 *      widening draws only bit 31, so under the shared tag no block of one is a block of another.
 *   3. noisy  iff  u < thr,  thr = min(2^32, ceil(noise * 2^32)): noise = 0 is never noisy, noise = 1 always.
 *   4. noisy: the action is crl_blokus_sample's at that counter -- its word under tag 0x424c0000, rank mulhi32(word, n).
 *      With noise = 1 the agent therefore is the random agent bit for bit.
 *   5. else the action is `best` of crl_blokus_mcts(cand = NULL, A = 1, W, S, R, cexp) on this position with tcount[b] taken
 *      as c; every draw of that search is exactly as its contract says.  The root always widens (no candidate roots).
 * Errors (CRL_EINVAL, with a crl_last_error message, before any device work; the context's check comes last): everything
 * the random sibling of each entry refuses, W outside [1, 64], S outside [1, S_max] (crl_blokus_mcts_max_simulations: the
 * same 1823 -- the word that hands `best` to the other waves of a workgroup fits the spare bytes of a tree's fixed part),
 * R outside [1, 1024], cexp > 65535, noise outside [0, 1] or NaN.
 * The tree lives in LDS with crl_blokus_mcts's layout and mappings: R < 4 one wave per game (up to four games per workgroup
 * as the trees fit), R >= 4 one workgroup per game, every wave replaying the game and the search's descents, wave 0 writing
 * the tree, the state and the outputs.  Both give the same bits.  The wave's LDS board is the search's scratch, so between
 * searches the wave keeps the position in registers; a noisy ply or a pass does not search.
 *
 * action[b] = the search agent's move at step counter tcount[b]; advance != 0 also increments tcount (passes included), as
 * crl_blokus_sample.  The state is read only. */
int crl_blokus_sample_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                           const uint32_t *inventory, const int32_t *score, const int32_t *round, const int32_t *to_move,
                           uint32_t *tcount, int advance, int W, int S, int R, uint32_t cexp, double noise,
                           int32_t *action, void *stream);
/* crl_blokus_rollout with EVERY seat on the search agent: the same auto-reset, crl_blokus_stats bookkeeping and results row,
 * the same checks of T (T = 0 launches nothing).  It has no launch-plan bind entry.
 * T x (crl_blokus_sample_mcts(advance = 1); crl_blokus_step with CRL_STEP_AUTO_RESET) == crl_blokus_rollout_mcts(T). */
int crl_blokus_rollout_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T, int W, int S, int R,
                            uint32_t cexp, double noise, uint32_t *occ, uint32_t *inv, int32_t *score, int32_t *round,
                            int32_t *to_move, crl_blokus_stats stats, void *stream);
/* crl_blokus_step_single word for word, except that in its step 2 the opponents' action is what
 * crl_blokus_sample_mcts(advance = 1) returns on that state -- the opponents who open a game that restarted inside the call
 * included: they search from the empty board.  The learner's ply (by id or by rank), the error codes that leave the game as
 * it was, and the reward, done, winners, n_valid and observation outputs are that entry's. */
int crl_blokus_step_single_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                                uint32_t *occ, uint32_t *inv, int32_t *score, int32_t *round, int32_t *to_move,
                                const int8_t *seat, const int64_t *learner_action, uint32_t *tcount,
                                int8_t *reward, uint8_t *done, uint8_t *winners, int32_t *n_valid,
                                int8_t *obs_board, uint8_t *obs_pieces, int32_t *obs_score,
                                int W, int S, int R, uint32_t cexp, double noise, uint32_t flags, void *stream);

/* ------------------------------------------------------------------ the tree search as a seated agent of TicTacToe
 * The search of crl_ttt_mcts in the three forms the random and the tactical agent have: one step, a fused rollout with
 * every seat on it, and the opponents of the single-player step.  Added under revision 113: new entries only, no new Philox
 * tag, no existing struct, argument list or RNG contract changed.
 * The search agent has the parameters S, R, cexp (crl_ttt_mcts's) and noise.  Its move for the mover p = to_move[b] at step
 * counter c of global game g = first_env_id + b, E the empty cells:
 *   1. p outside [0, P) or E == 0: the action is -1 (pass) and no draw is made (the tactical agent's rule 1).
 *   2. (u, v) are the tactical agent's two words at that counter, exactly its rule 2 for the entries that are no playouts:
 *      w = Philox4x32-10(ctr = {g, c >> 1, 0, 0x54630000}, key = {seed lo, seed hi}), u = w[2 (c & 1)], v = w[2 (c & 1) + 1].
 *      Only one agent moves at a given counter of a game, so the stream is shared at no cost.
 *   3. noisy  iff  u < thr,  thr = min(2^32, ceil(noise * 2^32)) as the tactical agent's rule 3: noise = 0 is never noisy,
 *      noise = 1 always.
 *   4. noisy: the action is the mulhi32(v, popcount(E))-th set bit of E, ascending -- with noise = 1 bit for bit the tactical
 *      agent at noise 1.
 *   5. else the action is `best` of crl_ttt_mcts(S, R, cexp) on this position with tcount[b] taken as c and winner[b] as -1
 *      (like crl_ttt_sample and the tactical agent, the agent reads occ and to_move only).  The playouts of that search draw
 *      as crl_ttt_mcts says: tag 0x544D0000, counter c + depth + k, third word (s << 16) | r.  With E != 0 and S >= 1 the
 *      root has a child, so `best` is an empty cell.
 * Errors (CRL_EINVAL, with a crl_last_error message, before any device work): everything the tactical sibling of each entry
 * refuses, S outside [1, S_max] (crl_ttt_mcts_max_simulations), R outside [1, 1024], cexp > 65535, noise outside [0, 1] or
 * NaN.
 * One wave per game, the tree in LDS with crl_ttt_mcts's layout (win-mask table, rank table, one tree per wave, one to four
 * waves per workgroup); outside the search the wave holds the game's position alike in every lane, and a noisy ply does not
 * search.  Games are walked in a grid-stride loop with 64-bit indices.
 *
 * action[b] = the search agent's move at step counter tcount[b]; advance != 0 also increments tcount (passes included). */
int crl_ttt_sample_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, const uint32_t *occ,
                        const int8_t *to_move, uint32_t *tcount, int advance, int S, int R, uint32_t cexp, double noise,
                        int8_t *action, void *stream);
/* crl_ttt_rollout_tactical with EVERY seat on the search agent: the same auto-reset, crl_ttt_stats bookkeeping and results
 * row, the same checks of T.
 * T x (crl_ttt_sample_mcts(advance = 1); crl_ttt_step with CRL_STEP_AUTO_RESET) == crl_ttt_rollout_mcts(T). */
int crl_ttt_rollout_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id, int T, int S, int R,
                         uint32_t cexp, double noise, uint32_t *occ, int8_t *winner, int8_t *to_move, crl_ttt_stats stats,
                         void *stream);
/* crl_ttt_step_single word for word, except that in its step 2 the opponents' action is what
 * crl_ttt_sample_mcts(advance = 1) returns on that state -- the opponents who open a game that was reset inside the call
 * included: they search from the empty board.  The learner's ply still consumes one counter value.  The learner's
 * observation is written with the wave's lanes as the cells. */
int crl_ttt_step_single_mcts(const crl_ctx *ctx, int64_t B, uint64_t seed, uint64_t first_env_id,
                             uint32_t *occ, int8_t *winner, int8_t *to_move, const int8_t *seat,
                             const int64_t *learner_action, uint32_t *tcount,
                             int8_t *reward, uint8_t *done, int8_t *winners,
                             int8_t *obs_board, uint32_t *valid, int rel_mod, int S, int R, uint32_t cexp, double noise,
                             uint32_t flags, void *stream);

/* ------------------------------------------------------------------ launch plans: bind a rollout's arguments once
 * A caller that launches short rollouts in a loop passes the same context, batch, state and statistics pointers and flags
 * every time; only the seed, the number of steps and the stream change.  A plan holds the constant part: a bind entry runs
 * every check of its rollout entry (context, B, NULL pointers, alignment, flags, statistics -- same codes, messages under the
 * bind entry's name, nothing touches the device) and stores the arguments with the launch geometry that does not depend on
 * T.  crl_rollout_launch then checks T (0 .. 2^24; T = 0 returns CRL_OK and launches nothing) and issues exactly the
 * launches the rollout entry issues for the same arguments -- the same kernel choice per T, the same split of long Tron
 * rollouts -- so the results are bit-identical and the call is as asynchronous and graph-capturable as that entry.
 * Added under revision 113: new entries only, no existing struct, argument list or RNG contract changed.
 * Lifetime: a plan refers to its context and to the caller's buffers; unbind it before crl_destroy of the context, and bind
 * a new one when a buffer moves.  A plan is immutable after bind: any number of host threads may launch one plan
 * concurrently (on different streams, or ordered by the stream they share).  crl_rollout_unbind frees a plan once no
 * launch call on it is in progress (launches already queued on a stream keep nothing of the plan); NULL is harmless.
 * Errors of crl_rollout_launch (CRL_EINVAL): a NULL plan, T outside the range; CRL_EHIP as the rollout entries. */
typedef struct crl_plan crl_plan;   /* opaque, immutable after bind */
int crl_tron_rollout_bind(const crl_ctx *ctx, int64_t B, uint64_t first_env_id,
                          int8_t *board, int16_t *heads, int8_t *dirs, int8_t *deaths,
                          crl_tron_stats stats, uint32_t flags, crl_plan **plan);
int crl_ttt_rollout_bind(const crl_ctx *ctx, int64_t B, uint64_t first_env_id,
                         uint32_t *occ, int8_t *winner, int8_t *to_move, crl_ttt_stats stats, crl_plan **plan);
int crl_blokus_rollout_bind(const crl_ctx *ctx, int64_t B, uint64_t first_env_id,
                            uint32_t *occ, uint32_t *inv, int32_t *score, int32_t *round, int32_t *to_move,
                            crl_blokus_stats stats, crl_plan **plan);
int crl_rollout_launch(const crl_plan *plan, uint64_t seed, int T, void *stream);
int crl_rollout_unbind(crl_plan *plan);

#ifdef __cplusplus
}
#endif
#endif
